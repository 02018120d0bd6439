"""CLI-level synthesis time, mel arrays in memory -> 16-bit PCM arrays in memory: the host path against ``--device_rng``.

    python tools/bench_synth.py --out profiles/device_synthesis.json

The workload is ``tools/bench_ragged.py``'s: the full model (hparams.py defaults, synthetic weights) and its 64 mel lengths of
200 - 900 frames (``FRAMES``), mels drawn from a seeded generator.  Four legs, each the loop the ``synthesize`` CLI runs with
the file writes replaced by keeping the PCM array:

  host           z from ``torch.randn`` on one CPU generator, fp32 up, ``reverse``, fp32 down, ``write_wav``'s float64 NumPy
                 clip / scale / round / cast; clips of equal length share a call
  host_ragged    the same per ``plan_batches`` group, one CPU generator per clip (``--ragged``)
  device         ``synthesize.synthesize_device``: mel up, ``FloWaveNet.synthesize``, int16 down into pinned memory, the next call
                 enqueued before the previous one's PCM is taken (``--device_rng``)
  device_ragged  the same over ``plan_batches`` groups (``--device_rng --ragged``)

One untimed round first, then ``--rounds`` rounds that run the four legs one after the other (alternating them: other people's
work shares the host); a leg's figure is the median of its rounds, host wall clock around work that ends with every PCM array
in host memory.  Reads nothing outside the repository.  A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ragged import FRAMES, FRAMES_SEED  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max_pad_frac", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=len(FRAMES), help="use the first N utterances only (rehearsals)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_synth.py measures on the GPU: none found")
    from tf_flowavenet_amd import synthesize as S, weights as W
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.model import FloWaveNet
    hp = default_hparams()
    hop = hp.hop_size
    frames = FRAMES[:args.clips]
    rng = np.random.default_rng(FRAMES_SEED)
    mels = [rng.random((f, hp.num_mels), dtype=np.float32) for f in frames]
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    seed = 75

    def to_pcm(audio):                               # synthesize.write_wav's arithmetic
        return (np.clip(np.asarray(audio, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")

    def host(out):                                   # synthesize.synthesize without --ragged
        by_len = {}
        for k, f in enumerate(frames):
            by_len.setdefault(f, []).append(k)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for f, group in sorted(by_len.items()):
            fa = S._aligned_frames(f, hp)
            per_call = min(args.batch, S.max_clips_per_call(hp, fa * hop))
            for i in range(0, len(group), per_call):
                chunk = group[i:i + per_call]
                c = np.stack([np.pad(mels[k], ((0, fa - f), (0, 0)), mode="edge") for k in chunk])
                z = torch.randn(len(chunk), fa * hop, 1, generator=gen) * hp.temp
                wav = model.reverse(z.cuda(), torch.from_numpy(c).cuda()).squeeze(-1).cpu().numpy()
                for k, w in zip(chunk, wav):
                    out[k] = to_pcm(w[:f * hop])

    def host_ragged(out):                            # synthesize._synthesize_ragged
        for group in S.plan_batches(frames, args.batch, args.max_pad_frac, hp):
            own = [S._aligned_frames(frames[k], hp) for k in group]
            top = max(own)
            c = np.zeros((len(group), top, hp.num_mels), dtype=np.float32)
            z = torch.zeros(len(group), top * hop, 1)
            for row, (k, f) in enumerate(zip(group, own)):
                c[row, :f] = np.pad(mels[k], ((0, f - frames[k]), (0, 0)), mode="edge")
                gen = torch.Generator(device="cpu").manual_seed(seed + k)
                z[row, :f * hop] = torch.randn(f * hop, 1, generator=gen) * hp.temp
            wav = model.reverse(z.cuda(), torch.from_numpy(c).cuda(), lengths=[f * hop for f in own]).squeeze(-1).cpu().numpy()
            for row, k in enumerate(group):
                out[k] = to_pcm(wav[row, :frames[k] * hop])

    def device(ragged):
        cfg = type("A", (), dict(batch=args.batch, ragged=ragged, max_pad_frac=args.max_pad_frac))()

        def run(out):
            groups = S.device_batches(frames, cfg, hp)
            S.synthesize_device(model, hp, mels, groups, seed, ragged, lambda k, pcm: out.__setitem__(k, np.array(pcm)))
        return run

    legs = [("host", host), ("host_ragged", host_ragged), ("device", device(False)), ("device_ragged", device(True))]
    times = {name: [] for name, _ in legs}
    for rnd in range(args.rounds + 1):               # round 0 warms every shape up and is not counted
        for name, fn in legs:
            out = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(out)
            dt = time.perf_counter() - t0
            assert sorted(out) == list(range(len(frames))) and all(out[k].dtype == np.int16 and out[k].size == frames[k] * hop for k in out)
            assert all(np.abs(out[k]).max() > 0 for k in out)
            if rnd:
                times[name].append(dt)
            print("round %d %-14s %.4f s" % (rnd, name, dt), flush=True)
    audio_s = sum(frames) * hop / float(hp.sample_rate)
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "frames_seed": FRAMES_SEED, "clips": len(frames),
           "samples": sum(frames) * hop, "audio_seconds": audio_s, "batch": args.batch, "max_pad_frac": args.max_pad_frac,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "host wall clock, mels in memory -> PCM arrays in memory; "
                      "median of the rounds, the legs alternating within a round"},
           "calls": {"equal_lengths": len(S.device_batches(frames, type("A", (), dict(batch=args.batch, ragged=False))(), hp)),
                     "ragged": len(S.plan_batches(frames, args.batch, args.max_pad_frac, hp))}}
    for name, _ in legs:
        med = statistics.median(times[name])
        res[name] = {"total_s": med, "total_s_min": min(times[name]), "total_s_max": max(times[name]),
                     "ms_per_utterance": 1e3 * med / len(frames), "times_real_time": audio_s / med, "rounds_s": [round(t, 5) for t in times[name]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["ms_per_utterance"] if isinstance(v, dict) and "ms_per_utterance" in v else v) for k, v in res.items()
                      if k in ("label", "gpu", "host", "host_ragged", "device", "device_ragged")}))


if __name__ == "__main__":
    main()
