"""The spectral denoiser on one MI355X:

    python tools/bench_denoise.py --out profiles/denoise.json

  (a) one ragged ``Denoiser`` call over the 64 utterances of 200 - 900 mel frames of ``tools/bench_synth.py`` (``FRAMES``; seeded
      noise of the clips' lengths, float32 on the device) to 16-bit PCM, timed by device events around the call: time, the bytes
      the call has to move (every clip's own samples in, every row of int16 out, the bias once), that as a share of the HBM
      rate given by ``--hbm_gbs``, and STFT frames per second;
  (b) the synthesis loop of ``synthesize --device_rng --ragged`` (``synthesize.synthesize_device``: mels in memory -> PCM arrays in
      memory, the full model with synthetic weights) with and without the denoiser, host wall clock: the share it adds;
  (c) the same clips through ``scipy.signal.stft`` / ``istft`` with the same window and the same threshold, 16 threads over the
      clips, host wall clock - the CPU baseline, in the same run;
  (d) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds.  Reads nothing outside the repository.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ragged import FRAMES, FRAMES_SEED  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=len(FRAMES), help="use the first N utterances only (rehearsals)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max_pad_frac", type=float, default=0.25)
    ap.add_argument("--strength", type=float, default=0.1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--hbm_gbs", type=float, default=8000.0, help="the HBM rate the share is taken of (MI355X data sheet: 8 TB/s)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise.py measures on the GPU: none found")
    from scipy.signal import istft, stft
    from tf_flowavenet_amd import synthesize as S, weights as W
    from tf_flowavenet_amd.denoise import Denoiser
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.model import FloWaveNet
    hp = default_hparams()
    hop, n_fft = hp.hop_size, hp.n_fft
    frames = FRAMES[:args.clips]
    rng = np.random.default_rng(FRAMES_SEED)
    mels = [rng.random((f, hp.num_mels), dtype=np.float32) for f in frames]
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    dn = Denoiser(model, strength=args.strength)
    bias = dn.bias.cpu().numpy().astype(np.float64)

    # (a) / (c): the clips
    lens = [f * hop for f in frames]
    top = max(lens)
    host = np.zeros((len(lens), top), dtype=np.float32)
    for b, n in enumerate(lens):
        host[b, :n] = np.clip(rng.normal(0.0, 0.3, n), -1.0, 1.0)
    x = torch.from_numpy(host).cuda()
    lens_dev = torch.tensor(lens, dtype=torch.int64).cuda()
    moved = 4 * sum(lens) + 2 * len(lens) * top + 4 * dn.nb
    stft_frames = sum(1 + n // hop for n in lens)

    def device_call():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        y = dn(x, lengths=lens_dev, pcm=True)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3, y

    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)

    def scipy_clip(b):
        v = np.pad(host[b, :lens[b]].astype(np.float64), n_fft // 2, mode="reflect")
        _, _, Z = stft(v, window=w, nperseg=n_fft, noverlap=n_fft - hop, boundary=None, padded=False)
        t = (args.strength * bias / w.sum())[:, None]          # scipy scales by 1 / sum(w)
        mag = np.abs(Z)
        Z = Z * np.where(mag > t, 1.0 - t / np.maximum(mag, 1e-300), 0.0)
        _, y = istft(Z, window=w, nperseg=n_fft, noverlap=n_fft - hop, boundary=None)
        return y[n_fft // 2:n_fft // 2 + lens[b]]

    def scipy_call():
        t0 = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as pool:
            ys = list(pool.map(scipy_clip, range(len(lens))))
        return time.perf_counter() - t0, ys

    # (b): the CLI's device loop
    cfg = type("A", (), dict(batch=args.batch, ragged=True, max_pad_frac=args.max_pad_frac))()
    groups = S.device_batches(frames, cfg, hp)

    def synth(denoiser):
        def run():
            out = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.synthesize_device(model, hp, mels, groups, 75, True, lambda k, pcm: out.__setitem__(k, np.array(pcm)), denoiser)
            dt = time.perf_counter() - t0
            assert sorted(out) == list(range(len(frames))) and all(out[k].dtype == np.int16 and out[k].size == lens[k] for k in out)
            return dt, out
        return run

    legs = [("device", device_call), ("scipy", scipy_call), ("synth_plain", synth(None)), ("synth_denoised", synth(dn))]
    times, last = {name: [] for name, _ in legs}, {}
    for rnd in range(args.rounds + 1):                   # round 0 warms up and is not counted
        for name, fn in legs:
            dt, last[name] = fn()
            if rnd:
                times[name].append(dt)
            print("round %d %-16s %.5f s" % (rnd, name, dt), flush=True)
    # the two legs computed the same thing (scipy's last frame differs where a clip's end does not fit a whole frame: the
    # comparison leaves the last n_fft samples out)
    y = last["device"].cpu().numpy()
    worst = max(int(np.abs(y[b, :lens[b] - n_fft].astype(np.int64)
                           - (np.clip(ref[:lens[b] - n_fft], -1.0, 1.0) * 32767.0).round().astype(np.int64)).max())
                for b, ref in enumerate(last["scipy"]))

    def stats(ts):
        return {"s": statistics.median(ts), "s_min": min(ts), "s_max": max(ts), "rounds_s": [round(t, 6) for t in ts]}

    dev, cpu, plain, den = (stats(times[k]) for k in ("device", "scipy", "synth_plain", "synth_denoised"))
    audio_s = sum(lens) / float(hp.sample_rate)
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "frames_seed": FRAMES_SEED,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "median of the rounds, the legs alternating within a round; "
                      "device: HIP events around the call; scipy and the synthesis loops: host wall clock"},
           "ragged_call": dict(dev, clips=len(lens), n_fft=n_fft, hop=hop, strength=args.strength, input_samples=sum(lens),
                               longest_clip=top, stft_frames=stft_frames, audio_seconds=audio_s, bytes_moved=moved,
                               gb_per_s=moved / dev["s"] * 1e-9, hbm_rate_assumed_gb_per_s=args.hbm_gbs,
                               share_of_hbm_rate=moved / dev["s"] * 1e-9 / args.hbm_gbs, frames_per_s=stft_frames / dev["s"],
                               times_real_time=audio_s / dev["s"], max_pcm_lsb_diff_from_scipy=worst),
           "scipy_stft_istft": dict(cpu, threads=args.threads, times_real_time=audio_s / cpu["s"], device_speedup=cpu["s"] / dev["s"]),
           "synthesis_device_rng_ragged": {"calls": len(groups), "batch": args.batch, "max_pad_frac": args.max_pad_frac,
                                           "plain": plain, "denoised": den, "added_share": den["s"] / plain["s"] - 1.0},
           "default_path": "NOT MEASURED by this tool: python bench.py on this commit against its parent"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"device_s": dev["s"], "gb_per_s": res["ragged_call"]["gb_per_s"], "frames_per_s": res["ragged_call"]["frames_per_s"],
                      "scipy_s": cpu["s"], "synth_plain_s": plain["s"], "synth_denoised_s": den["s"],
                      "max_pcm_lsb_diff_from_scipy": worst}))


if __name__ == "__main__":
    main()
