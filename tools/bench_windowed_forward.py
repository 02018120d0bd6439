"""Windowed forward on one MI355X, the full model (hparams.py defaults, synthetic weights), audio and mel on the device ->
per-clip (log_p, logdet) on the device:

    python tools/bench_windowed_forward.py --out profiles/windowed_forward.json

  (a) one clip of 3 932 160 samples (below what one call addresses): ``FloWaveNet.forward`` in one call against
      ``forward_windowed`` at windows 65 536, 262 144 and 1 048 576, ``--batch`` windows per call; beside each the rows run over
      the clip's rows - what the halos cost - and, with ``return_z``, the same legs again with the time-ordered latent;
  (b) one 30-minute clip (39 689 984 samples) at window 262 144, windowed only, on a model of its own: total time, and from
      the cold round the call's own peak footprint (its workspaces - a function of batch and window alone -, the tables and the
      per-window sums) beside the bytes of the clip's audio and mel;
  (c) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds, host wall clock around work that ends with ``torch.cuda.synchronize()``.
The one-call forward runs the chained and one-launch forms of the pass, the windows the launch-per-stage form that keeps every
tail's ZeroConv output: the comparison is of the two paths as they are.  Reads nothing outside the repository.  A run without a
GPU fails."""
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
        raise SystemExit("bench_windowed_forward.py measures on the GPU: none found")
    from tf_flowavenet_amd import weights as W, windowing as WIN
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.model import FloWaveNet
    hp = default_hparams()
    hop, unit, halo = hp.hop_size, WIN.unit_samples(hp), WIN.halo_samples(hp)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    gen = torch.Generator(device="cuda").manual_seed(0)

    def clip_of(samples):
        return (0.3 * torch.randn(1, samples, 1, device="cuda", generator=gen),
                torch.rand(1, samples // hop, hp.num_mels, device="cuda", generator=gen))

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
    x_a, c_a = clip_of(t_a)
    windows = (65536, 262144, 1048576)
    legs = [("one_call", lambda: model.forward(x_a, c_a)), ("one_call_z", lambda: model.forward(x_a, c_a, return_z=True))]
    for w in windows:
        legs.append(("window_%d" % w, (lambda w: lambda: model.forward_windowed(x_a, c_a, w, batch=args.batch))(w)))
        legs.append(("window_%d_z" % w, (lambda w: lambda: model.forward_windowed(x_a, c_a, w, batch=args.batch, return_z=True))(w)))
    # (b) the long clip (first in a round: in the cold round nothing but the two models and the two clips is allocated when it starts)
    t_b = int(args.long_minutes * 60 * hp.sample_rate) // unit * unit
    x_b, c_b = clip_of(t_b)
    model_b = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))     # its caches hold (b)'s shapes only
    legs.insert(0, ("long_clip", lambda: model_b.forward_windowed(x_b, c_b, 262144, batch=args.batch)))
    times = {name: [] for name, _ in legs}
    call_bytes, scalars = {}, {}
    for rnd in range(args.rounds + 1):               # round 0 warms every shape up and is not counted
        for name, fn in legs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            dt, out = timed(fn)
            assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
            scalars[name] = (float(out[0].reshape(-1)[0]), float(out[1].reshape(-1)[0]))
            if rnd == 0:                             # cold caches: the call allocates everything it needs
                call_bytes[name] = torch.cuda.max_memory_allocated() - before
            del out
            if rnd:
                times[name].append(dt)
            print("round %d %-18s %.4f s" % (rnd, name, dt), flush=True)
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "halo_samples": halo, "batch": args.batch,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "host wall clock, audio and mel on the device -> scalars (and z) "
                      "on the device, synchronised; median of the rounds, the legs alternating within a round"},
           "below_the_ceiling": {"samples": t_a},
           "long_clip": dict(stats(times["long_clip"], t_b), samples=t_b, minutes=t_b / hp.sample_rate / 60.0, window=262144,
                             call_peak_bytes=call_bytes["long_clip"], audio_bytes=t_b * 4, mel_bytes=c_b.numel() * 4,
                             log_p=scalars["long_clip"][0], logdet=scalars["long_clip"][1])}
    below = res["below_the_ceiling"]
    for name in ("one_call", "one_call_z"):
        below[name] = dict(stats(times[name], t_a), call_peak_bytes=call_bytes[name], log_p=scalars[name][0], logdet=scalars[name][1])
    for w in windows:
        plan = WIN.plan_windows(t_a, w, hp)
        for suffix in ("", "_z"):
            name = "window_%d%s" % (w, suffix)
            below[name] = dict(stats(times[name], t_a), rows_over_clip_rows=sum(hi - lo for lo, hi, _, _ in plan) / t_a,
                               rows_over_clip_rows_nominal=(w + 2 * halo) / w, calls=len(WIN.group_windows([plan], args.batch, hp)),
                               against_one_call=statistics.median(times[name]) / statistics.median(times["one_call" + suffix]),
                               call_peak_bytes=call_bytes[name], log_p=scalars[name][0], logdet=scalars[name][1])
    res["default_path"] = "NOT MEASURED by this tool: python bench.py on this commit against its parent"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"one_call_s": below["one_call"]["total_s"], **{"window_%d_s" % w: below["window_%d" % w]["total_s"] for w in windows},
                      "long_clip_s": res["long_clip"]["total_s"], "long_clip_call_peak_bytes": res["long_clip"]["call_peak_bytes"]}))


if __name__ == "__main__":
    main()
