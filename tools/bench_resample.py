"""Sample-rate conversion on one MI355X:

    python tools/bench_resample.py --out profiles/resample.json

  (a) one ragged ``Resampler`` call over 64 clips of 2 to 10 s at 48 kHz -> 22 050 Hz (seeded lengths, float32 on the device),
      timed by device events around the call: time, the bytes the call has to move (every clip's own samples in, every row of
      the output out, the phase table once) and that as a share of the HBM rate given by ``--hbm_gbs``;
  (b) the same clips through ``scipy.signal.resample_poly`` with the same taps (``window=h / up``, ``padtype="constant"``:
      the same sums in fp64), 16 threads over the clips, host wall clock - the CPU baseline, in the same run;
  (c) ``preprocessing.preprocess`` on a seeded corpus of ``--utterances`` 16-bit wavs of 2 to 6 s written at 48 kHz against
      the same signals written at 22 050 Hz (no resampling): host wall clock, files written to a temporary directory;
  (d) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds.  Reads nothing outside the repository.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave
from concurrent.futures import ThreadPoolExecutor


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--utterances", type=int, default=24)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--hbm_gbs", type=float, default=8000.0, help="the HBM rate the share is taken of (MI355X data sheet: 8 TB/s)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU: none found")
    from scipy.signal import resample_poly
    sys.path.insert(0, os.path.join(args.root, "tests"))
    import resample_ref as R
    from tf_flowavenet_amd import preprocessing as P
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.resample import Resampler
    hp = default_hparams()
    in_rate, out_rate = 48000, hp.sample_rate
    rng = np.random.default_rng(1234)

    # (a) / (b): the clips
    lens = [int(v) for v in rng.integers(2 * in_rate, 10 * in_rate + 1, args.clips)]
    top = max(lens)
    host = np.zeros((args.clips, top), dtype=np.float32)
    for b, n in enumerate(lens):
        host[b, :n] = rng.uniform(-0.5, 0.5, n)
    rs = Resampler(in_rate, out_rate)
    x = torch.from_numpy(host).cuda()
    lens_dev = torch.tensor(lens, dtype=torch.int64).cuda()
    n_out = rs.out_length(top)
    moved = 4 * sum(lens) + 4 * args.clips * n_out + 4 * rs.up * rs.taps
    h = R.design(rs.up, rs.down)

    def device_call():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        y = rs(x, lengths=lens_dev)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3, y

    def scipy_call():
        t0 = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as pool:
            ys = list(pool.map(lambda b: resample_poly(host[b, :lens[b]].astype(np.float64), rs.up, rs.down, window=h / rs.up,
                                                       padtype="constant"), range(args.clips)))
        return time.perf_counter() - t0, ys

    # (c): the corpora
    tmp = tempfile.TemporaryDirectory()
    corpora = {}
    for rate in (in_rate, out_rate):
        book = os.path.join(tmp.name, "in%d" % rate, "book1")
        os.makedirs(os.path.join(book, "wavs"))
        urng = np.random.default_rng(99)                 # the same signals at either rate: seconds and tones, then noise
        for u in range(args.utterances):
            secs, f0 = float(urng.uniform(2.0, 6.0)), float(urng.uniform(100.0, 300.0))
            t = np.arange(int(secs * rate)) / float(rate)
            sig = 0.4 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 7.3 * f0 * t) + 0.02 * urng.standard_normal(len(t))
            with wave.open(os.path.join(book, "wavs", "u%03d.wav" % u), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(rate)
                w.writeframes(np.round(sig * 32767.0).astype("<i2").tobytes())
        with open(os.path.join(book, "metadata.csv"), "w", encoding="utf-8") as f:
            f.write("\n".join("u%03d|t|t" % u for u in range(args.utterances)))
        corpora[rate] = os.path.join(tmp.name, "in%d" % rate)

    def preprocess_call(rate):
        def run():
            out = tempfile.mkdtemp(dir=tmp.name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as null:
                stdout, sys.stdout = sys.stdout, null
                try:
                    meta = P.preprocess(corpora[rate], out, hp)
                finally:
                    sys.stdout = stdout
            torch.cuda.synchronize()
            return time.perf_counter() - t0, sum(m[2] for m in meta)
        return run

    legs = [("device", device_call), ("scipy", scipy_call), ("preprocess_48000", preprocess_call(in_rate)),
            ("preprocess_22050", preprocess_call(out_rate))]
    times, last = {name: [] for name, _ in legs}, {}
    for rnd in range(args.rounds + 1):                   # round 0 warms up and is not counted
        for name, fn in legs:
            dt, last[name] = fn()
            if rnd:
                times[name].append(dt)
            print("round %d %-18s %.5f s" % (rnd, name, dt), flush=True)
    # the two legs computed the same thing
    y = last["device"].cpu().numpy()
    worst = max(float(np.abs(y[b, :len(ref)] - ref).max()) for b, ref in enumerate(last["scipy"]))

    def stats(ts):
        return {"s": statistics.median(ts), "s_min": min(ts), "s_max": max(ts), "rounds_s": [round(t, 6) for t in ts]}

    dev, cpu = stats(times["device"]), stats(times["scipy"])
    audio_s = sum(lens) / float(in_rate)
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0),
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "median of the rounds, the legs alternating within a round; "
                      "device: HIP events around the call; scipy and preprocess: host wall clock"},
           "ragged_call": dict(dev, clips=args.clips, in_rate=in_rate, out_rate=out_rate, up=rs.up, down=rs.down, taps_per_output=rs.taps,
                               table_bytes=4 * rs.up * rs.taps, input_samples=sum(lens), longest_clip=top, output_row=n_out,
                               audio_seconds=audio_s, bytes_moved=moved, gb_per_s=moved / dev["s"] * 1e-9,
                               hbm_rate_assumed_gb_per_s=args.hbm_gbs, share_of_hbm_rate=moved / dev["s"] * 1e-9 / args.hbm_gbs,
                               times_real_time=audio_s / dev["s"], max_abs_diff_from_scipy=worst),
           "scipy_resample_poly": dict(cpu, threads=args.threads, times_real_time=audio_s / cpu["s"], device_speedup=cpu["s"] / dev["s"]),
           "preprocess": {"utterances": args.utterances, "samples_written": last["preprocess_22050"],
                          "corpus_48000": stats(times["preprocess_48000"]), "corpus_22050": stats(times["preprocess_22050"]),
                          "ratio": statistics.median(times["preprocess_48000"]) / statistics.median(times["preprocess_22050"])},
           "default_path": "NOT MEASURED by this tool: python bench.py on this commit against its parent"}
    tmp.cleanup()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"device_s": dev["s"], "share_of_hbm_rate": res["ragged_call"]["share_of_hbm_rate"], "scipy_s": cpu["s"],
                      "preprocess_48000_s": res["preprocess"]["corpus_48000"]["s"],
                      "preprocess_22050_s": res["preprocess"]["corpus_22050"]["s"], "max_abs_diff_from_scipy": worst}))


if __name__ == "__main__":
    main()
