"""Synthesis of a directory of utterances of different lengths: one ``reverse`` per clip against ragged batches.

    python tools/bench_ragged.py --legs single,ragged,mask --label <commit> --out profiles/ragged_synthesis.part.json

The workload is fixed: the full model (hparams.py defaults, synthetic weights) and 64 mel lengths drawn uniformly from
200 - 900 frames (``FRAMES``, ``numpy.random.default_rng(FRAMES_SEED).integers(200, 901, 64)``).

  single   one plain ``reverse`` per clip (B = 1, T = frames * hop).  Uses nothing this feature added, so the same file
           runs on a checkout of the parent commit (``--root <that checkout>``): that run is the baseline.
  ragged   ``synthesize.plan_batches(FRAMES, --batch, --max_pad_frac)`` and one ``reverse(..., lengths=)`` per group.
  mask     one B = 8, T = 16 128 call on a ``chain_mode=1, persist_mode=1`` model (no chaining, no one-launch flows:
           the stage sequence a ragged pass runs), through the C entry points with the lengths already on the device:
           ``fwn_model_reverse`` against ``fwn_model_reverse_ragged`` with every length = T.  The masks zero nothing
           there, so the difference is what their launches cost.

Every figure is the median over ``--repeats`` windows of ``--inner`` back-to-back calls between two device events, after
``--warmup`` untimed calls of the same shape; the legs' totals are sums of the per-call medians.  A run without a GPU
fails."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

FRAMES_SEED = 20261017
FRAMES = [781, 780, 585, 555, 800, 871, 243, 739, 666, 583, 813, 674, 222, 454, 276, 470, 247, 390, 516, 553, 696, 395, 573, 595,
          775, 806, 642, 698, 505, 242, 253, 557, 649, 857, 283, 293, 390, 781, 240, 442, 545, 651, 615, 377, 781, 881, 552, 332,
          530, 482, 424, 689, 329, 368, 211, 243, 332, 316, 202, 306, 700, 449, 828, 698]


def timed(fn, warmup, repeats, inner):
    """Median milliseconds of one fn() over `repeats` event-timed windows of `inner` calls, and the windows' spread."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="single,ragged,mask")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max_pad_frac", type=float, default=0.25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    assert args.repeats >= 5
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    assert np.random.default_rng(FRAMES_SEED).integers(200, 901, size=64).tolist() == FRAMES
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on the GPU: none found")
    from tf_flowavenet_amd import _lib, synthesize as S, weights as W
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.model import FloWaveNet
    hp = default_hparams()
    hop = hp.hop_size
    params = W.synthetic_params(hp, 1234, actnorm="random")
    res = {"label": args.label, "device": torch.cuda.get_device_name(0), "frames_seed": FRAMES_SEED, "clips": len(FRAMES),
           "samples": sum(FRAMES) * hop, "timing": {"warmup": args.warmup, "repeats": args.repeats, "inner": args.inner,
                                                    "clock": "device events, median of the windows"}}
    legs = args.legs.split(",")
    gen = torch.Generator(device="cpu").manual_seed(75)

    def inputs(b, t):
        z = (torch.randn(b, t, 1, generator=gen) * hp.temp).cuda()
        c = torch.rand(b, t // hop, hp.num_mels, generator=gen).cuda()
        return z, c

    if "single" in legs or "ragged" in legs:
        model = FloWaveNet(hp).load_params(params)
    if "single" in legs:
        per = []
        for f in FRAMES:
            z, c = inputs(1, f * hop)
            per.append(timed(lambda: model.reverse(z, c), args.warmup, args.repeats, args.inner))
        res["single"] = {"calls": len(per), "total_ms": sum(p[0] for p in per), "total_ms_min": sum(p[1] for p in per),
                         "total_ms_max": sum(p[2] for p in per), "per_call_ms": [round(p[0], 4) for p in per]}
        print("single: %d calls, %.2f ms" % (len(per), res["single"]["total_ms"]), flush=True)
    if "ragged" in legs:
        groups = S.plan_batches(FRAMES, args.batch, args.max_pad_frac, hp)
        per, pad, tot = [], 0, 0
        for g in groups:
            lens = [FRAMES[k] * hop for k in g]
            z, c = inputs(len(g), max(lens))
            per.append(timed(lambda: model.reverse(z, c, lengths=lens), args.warmup, args.repeats, args.inner))
            pad += len(g) * max(lens) - sum(lens)
            tot += len(g) * max(lens)
        res["ragged"] = {"batch": args.batch, "max_pad_frac": args.max_pad_frac, "calls": len(groups), "group_sizes": [len(g) for g in groups],
                         "padding_share": pad / tot, "total_ms": sum(p[0] for p in per), "total_ms_min": sum(p[1] for p in per),
                         "total_ms_max": sum(p[2] for p in per), "per_call_ms": [round(p[0], 4) for p in per]}
        print("ragged: %d calls, %.2f ms (padding %.1f %%)" % (len(groups), res["ragged"]["total_ms"], 100.0 * pad / tot), flush=True)
    if "mask" in legs:
        b, t = 8, 16128
        m2 = FloWaveNet(hp, chain_mode=1, persist_mode=1).load_params(params)
        z, c = inputs(b, t)
        lib, md, st = _lib.load(), C.byref(m2._packed.model_desc), m2._stream()
        x = torch.empty(b, t, 1, device="cuda")
        ld = torch.tensor([t] * b, dtype=torch.int32).cuda()
        wp, wn = m2._workspace(b, t)
        rp, rn = m2._workspace(b, t, ragged=True)

        def plain():
            _lib.check(lib.fwn_model_reverse(md, b, t, z.data_ptr(), c.data_ptr(), wp, wn, x.data_ptr(), st))

        def ragged():
            _lib.check(lib.fwn_model_reverse_ragged(md, b, t, z.data_ptr(), c.data_ptr(), ld.data_ptr(), rp, rn, x.data_ptr(), st))

        plain()
        ref = x.clone()
        ragged()
        assert torch.equal(ref, x), "full lengths must change no bit"
        rows = []
        for _ in range(3):                        # alternate the two: other people's work shares the host
            rows.append((timed(plain, args.warmup, args.repeats, 4 * args.inner), timed(ragged, args.warmup, args.repeats, 4 * args.inner)))
        p_ms = statistics.median(r[0][0] for r in rows)
        r_ms = statistics.median(r[1][0] for r in rows)
        py = timed(lambda: m2.reverse(z, c, lengths=[t] * b), args.warmup, args.repeats, 4 * args.inner)
        n_masks = 1 + (len(hp.upsample_scales) - 1) + 1 + hp.n_block * hp.n_flow * (hp.n_layer + 1) + 1
        res["mask"] = {"B": b, "T": t, "plain_ms": p_ms, "ragged_full_lengths_ms": r_ms, "mask_cost_ms": r_ms - p_ms,
                       "mask_launches": n_masks, "rounds": [[r[0][0], r[1][0]] for r in rows],
                       "python_reverse_with_lengths_ms": py[0]}
        print("mask: plain %.4f ms, ragged with full lengths %.4f ms, %d mask launches cost %.4f ms" % (p_ms, r_ms, n_masks, r_ms - p_ms),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k in ("label", "device")}))


if __name__ == "__main__":
    main()
