"""Windowed synthesis on one MI355X, the full model (hparams.py defaults, synthetic weights), mel on the device -> 16-bit PCM on
the device:

    python tools/bench_windowed.py --out profiles/windowed_synthesis.json

  (a) one clip of 3 932 160 samples (below what one call addresses): ``FloWaveNet.synthesize`` in one call against
      ``synthesize_windowed`` at windows 65 536, 262 144 and 1 048 576, ``--batch`` windows per call; beside each the row overhead
      (window + 2 H) / window - what the halos cost in rows run through the network;
  (b) one 30-minute clip (39 689 984 samples), windowed only, on a model of its own: total time, and from the cold round
      ``torch.cuda.max_memory_allocated`` (two models and both legs' mels included) and that minus what was allocated before the call - the call's own footprint: its workspaces
      (a function of batch and window alone), the tables and the clip's PCM - beside the bytes of the clip's mel and PCM;
  (c) ``FloWaveNet.stream`` at windows 16 384 and 65 536: host time from the push that completes a window to that window's PCM
      on the host, frames pushed 64 at a time;
  (d) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds, host wall clock around work that ends with ``torch.cuda.synchronize()``.
Reads nothing outside the repository.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long_minutes", type=float, default=30.0, help="length of the clip of (b)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_windowed.py measures on the GPU: none found")
    from tf_flowavenet_amd import weights as W, windowing as WIN
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.model import FloWaveNet
    hp = default_hparams()
    hop, unit, halo = hp.hop_size, WIN.unit_samples(hp), WIN.halo_samples(hp)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    seed = 75
    gen = torch.Generator(device="cuda").manual_seed(0)

    def mel_of(samples):
        return torch.rand(1, samples // hop, hp.num_mels, device="cuda", generator=gen)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def stats(ts, samples):
        med = statistics.median(ts)
        return {"total_s": med, "total_s_min": min(ts), "total_s_max": max(ts), "times_real_time": samples / hp.sample_rate / med,
                "rounds_s": [round(t, 5) for t in ts]}

    # (a) below the ceiling: one call against windows
    t_a = 3932160
    c_a = mel_of(t_a)
    windows = (65536, 262144, 1048576)
    legs = [("one_call", lambda: model.synthesize(c_a, seed))]
    legs += [("window_%d" % w, (lambda w: lambda: model.synthesize_windowed(c_a, seed, window=w, batch=args.batch))(w)) for w in windows]
    # (b) the long clip
    t_b = int(args.long_minutes * 60 * hp.sample_rate) // unit * unit
    c_b = mel_of(t_b)
    model_b = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))     # its caches hold (b)'s shapes only
    # (first in a round: in the cold round nothing but the two models and the two mels is allocated when it starts)
    legs.insert(0, ("long_clip", lambda: model_b.synthesize_windowed(c_b, seed, window=262144, batch=args.batch)))
    times = {name: [] for name, _ in legs}
    call_bytes, abs_peak = {}, {}
    for rnd in range(args.rounds + 1):               # round 0 warms every shape up and is not counted
        for name, fn in legs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            dt, pcm = timed(fn)
            assert pcm.dtype == torch.int16 and int(pcm.abs().max()) > 0
            if rnd == 0:                             # cold caches: the call allocates everything it needs
                abs_peak[name] = torch.cuda.max_memory_allocated()
                call_bytes[name] = abs_peak[name] - before
            del pcm
            if rnd:
                times[name].append(dt)
            print("round %d %-16s %.4f s" % (rnd, name, dt), flush=True)
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "halo_samples": halo, "batch": args.batch,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "host wall clock, mel on the device -> PCM on the device, "
                      "synchronised; median of the rounds, the legs alternating within a round"},
           "below_the_ceiling": {"samples": t_a, "one_call": stats(times["one_call"], t_a)},
           "long_clip": dict(stats(times["long_clip"], t_b), samples=t_b, minutes=t_b / hp.sample_rate / 60.0, window=262144,
                             call_peak_bytes=call_bytes["long_clip"], max_memory_allocated_bytes=abs_peak["long_clip"], mel_bytes=c_b.numel() * 4, pcm_bytes=t_b * 2)}
    for w in windows:
        plan = WIN.plan_windows(t_a, w, hp)
        res["below_the_ceiling"]["window_%d" % w] = dict(
            stats(times["window_%d" % w], t_a), row_overhead_nominal=(w + 2 * halo) / w,
            row_overhead_actual=sum(hi - lo for lo, hi, _, _ in plan) / t_a, calls=len(WIN.group_windows([plan], args.batch, hp)),
            against_one_call=statistics.median(times["window_%d" % w]) / statistics.median(times["one_call"]),
            call_peak_bytes=call_bytes["window_%d" % w])
    res["below_the_ceiling"]["one_call"]["call_peak_bytes"] = call_bytes["one_call"]

    # (c) the stream: latency from the push that completes a window to its PCM on the host
    res["stream"] = {}
    for w in (16384, 65536):
        frames = (3 * w + 2 * halo) // hop
        c = mel_of(frames * hop)[0]
        lat = []
        for rnd in range(args.rounds + 1):
            st = model.stream(seed, window=w)
            for i in range(0, frames, 64):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pcm = st.push(c[i:i + 64])
                if pcm.numel():
                    host = pcm.cpu()
                    if rnd:
                        lat.append(time.perf_counter() - t0)
                    assert host.numel() % w == 0
            st.finish()
        res["stream"]["window_%d" % w] = {"push_to_pcm_on_host_s": statistics.median(lat), "min_s": min(lat), "max_s": max(lat),
                                          "window_audio_s": w / hp.sample_rate, "samples_per_call": w + 2 * halo, "measured_windows": len(lat)}
        print("stream window %d: %.4f s" % (w, statistics.median(lat)), flush=True)
    res["default_path"] = "NOT MEASURED by this tool: python bench.py on this commit against its parent"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"one_call_s": res["below_the_ceiling"]["one_call"]["total_s"],
                      **{"window_%d_s" % w: res["below_the_ceiling"]["window_%d" % w]["total_s"] for w in windows},
                      "long_clip_s": res["long_clip"]["total_s"], "long_clip_call_peak_bytes": res["long_clip"]["call_peak_bytes"]}))


if __name__ == "__main__":
    main()
