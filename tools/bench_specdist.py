"""The spectral distances (``metrics.SpectralDistance``, csrc/specdist.hip) on one MI355X:

    python tools/bench_specdist.py --out profiles/spectral_distance.json

over the 64 utterances of 200 - 900 mel frames of ``tools/bench_synth.py`` (``FRAMES``): seeded noise of the clips' lengths as the
targets, a perturbed copy of each as the test clip, both on the device as ``[64, longest]`` rows with their lengths.

  (a) ``SpectralDistance.dist`` at the model's resolution and at three (512/128, 1024/256, 2048/512), by device events around
      the call; the bytes the launches have to move (both clips' own samples per resolution, the filterbank once, the partials
      out and in, 32 bytes per clip out) and that as a share of the HBM rate given by ``--hbm_gbs``;
  (b) the share the one-resolution and three-resolution calls add to the ``synthesize --device_rng --ragged`` loop: the loop of
      ``tools/bench_synth.py``'s ``device_ragged`` leg (host wall clock, PCM arrays in host memory), and ``dist`` over the same
      ``plan_batches`` groups (device events; seeded noise of the groups' shapes stands for the waveforms);
  (c) the composition the call replaces, in the same run: ``MelFrontEnd(normalize=False)`` on both clips, ``torch.stft`` of both
      per resolution and the reductions in torch, frames past a clip's own masked out - by device events; the bytes its
      spectrograms take (written once and read once each, complex64).  Its numbers are the rectangle's: a clip's last frames
      reflect at the row's end, not at the clip's, so it is a timing leg, not a reference;
  (d) float32 NumPy / scipy (``scipy.fft.rfft(workers=16)``) per clip on the host, host wall clock;
  (e) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds.  Nothing is asserted about speed.  Reads nothing outside the repository.
A run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ragged import FRAMES, FRAMES_SEED  # noqa: E402

THREE = [(512, 128), (1024, 256), (2048, 512)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package runs")
    ap.add_argument("--label", default="", help="commit of that checkout (recorded)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=len(FRAMES), help="use the first N utterances only (rehearsals)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max_pad_frac", type=float, default=0.25)
    ap.add_argument("--threads", type=int, default=16, help="scipy.fft workers of the host leg")
    ap.add_argument("--hbm_gbs", type=float, default=8000.0, help="the HBM rate the share is taken of (MI355X data sheet: 8 TB/s)")
    ap.add_argument("--no_synth", action="store_true", help="skip the synthesis loop of (b) (rehearsals)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_specdist.py measures on the GPU: none found")
    from scipy.fft import rfft
    from tf_flowavenet_amd import preprocessing as P, synthesize as S, weights as W
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd.metrics import SpectralDistance
    hp = default_hparams()
    hop, M = hp.hop_size, hp.num_mels
    own = (hp.n_fft, hp.hop_size)
    frames = FRAMES[:args.clips]
    rng = np.random.default_rng(FRAMES_SEED)
    lens = [f * hop - 1 for f in frames]                 # 1 + N div hop = f frames at the model's hop
    ref = [np.clip(rng.normal(0.0, 0.3, n), -1.0, 1.0).astype(np.float32) for n in lens]
    test = [(np.float32(0.9) * c + np.float32(0.03) * rng.standard_normal(len(c)).astype(np.float32)).astype(np.float32) for c in ref]
    b, top = len(lens), max(lens)
    x, _ = P.ragged_rows(ref, "cuda")
    y, _ = P.ragged_rows(test, "cuda")
    lens_dev = torch.tensor(lens, dtype=torch.int64, device="cuda")
    sd1, sd3 = SpectralDistance(hp), SpectralDistance(hp, THREE)
    front = P.MelFrontEnd(hp)
    fb_np = P.mel_filterbank(hp)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3, out

    def call(sd):
        return lambda: timed(lambda: sd.dist(x, y, lengths=lens_dev))

    # (c) the composition in torch
    windows = {n: torch.hann_window(n, periodic=True, device="cuda") for n, _ in THREE}

    def composition(resolutions):
        def run():
            _, mx, _ = front(x, lengths=lens_dev, normalize=False, audio=False)
            _, my, _ = front(y, lengths=lens_dev, normalize=False, audio=False)
            f_own = 1 + lens_dev // hop
            live = (torch.arange(mx.shape[1], device="cuda")[None] < f_own[:, None]).double()
            out = {"mel_l1": ((mx - my).abs().double().sum(2) * live).sum(1) / (f_own * M)}
            lsd, sc = [], []
            for n_fft, h in resolutions:
                X = torch.stft(x, n_fft, h, window=windows[n_fft], center=True, pad_mode="reflect", return_complex=True)
                Y = torch.stft(y, n_fft, h, window=windows[n_fft], center=True, pad_mode="reflect", return_complex=True)
                px, py = X.real ** 2 + X.imag ** 2, Y.real ** 2 + Y.imag ** 2                  # [B, nb, F]
                f_b = 1 + lens_dev // h
                keep = (torch.arange(px.shape[2], device="cuda")[None] < f_b[:, None]).double()
                d = 10.0 * torch.log10(px.clamp_min(1e-4)) - 10.0 * torch.log10(py.clamp_min(1e-4))
                lsd.append(((d * d).double().mean(1).sqrt() * keep).sum(1) / f_b)
                num = (((px.sqrt() - py.sqrt()) ** 2).double().sum(1) * keep).sum(1)
                sc.append(num.sqrt() / (px.double().sum(1) * keep).sum(1).sqrt())
            out["lsd_db"], out["sc"] = sum(lsd) / len(lsd), sum(sc) / len(sc)
            return out
        return lambda: timed(run)

    # (d) float32 NumPy / scipy on the host
    def frames32(c, n_fft, h):
        n = len(c)
        j = np.arange(1 + n // h)[:, None] * h + np.arange(n_fft)[None, :] - n_fft // 2
        j = np.where(j < 0, -j, j)
        j = np.where(j >= n, 2 * (n - 1) - j, j)
        w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
        return c[j] * w[None, :]

    def power32(c, n_fft, h):
        X = rfft(frames32(c, n_fft, h), axis=1, workers=args.threads)
        return X.real * X.real + X.imag * X.imag

    def host(resolutions):
        def run():
            t0 = time.perf_counter()
            out = np.zeros((b, 3))
            lo, rf = np.float32(hp.min_level_db), np.float32(hp.ref_level_db)
            for k, (a, c) in enumerate(zip(ref, test)):
                lsd, sc = [], []
                for n_fft, h in resolutions:
                    px, py = power32(a, n_fft, h), power32(c, n_fft, h)
                    if (n_fft, h) == own:
                        ma, mc = (np.clip((np.float32(20) * np.log10(np.maximum(np.float32(1e-4), p @ fb_np.T)) - rf - lo) / -lo, 0, 1)
                                  for p in (px, py))
                        out[k, 0] = np.abs(ma - mc).astype(np.float64).mean()
                    d = np.float32(10) * np.log10(np.maximum(np.float32(1e-4), px)) - np.float32(10) * np.log10(np.maximum(np.float32(1e-4), py))
                    lsd.append(np.sqrt((d * d).astype(np.float64).mean(1)).mean())
                    m = np.sqrt(px) - np.sqrt(py)
                    sc.append(np.sqrt((m * m).astype(np.float64).sum()) / np.sqrt(px.astype(np.float64).sum()))
                out[k, 1], out[k, 2] = np.mean(lsd), np.mean(sc)
            return time.perf_counter() - t0, out
        return run

    # (b) the synthesis loop and the calls over its groups
    legs = [("call_1", call(sd1)), ("call_3", call(sd3)), ("torch_1", composition([own])), ("torch_3", composition(THREE)),
            ("numpy_1", host([own])), ("numpy_3", host(THREE))]
    groups = S.plan_batches(frames, args.batch, args.max_pad_frac, hp)
    if not args.no_synth:
        from tf_flowavenet_amd.model import FloWaveNet
        model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
        mels = [rng.random((f, M), dtype=np.float32) for f in frames]
        cfg = type("A", (), dict(batch=args.batch, ragged=True, max_pad_frac=args.max_pad_frac))()
        shapes = []
        for g in groups:
            own_f = [S._aligned_frames(frames[k], hp) for k in g]
            t = max(own_f) * hop
            shapes.append((torch.randn(len(g), t, device="cuda") * 0.3, torch.randn(len(g), t, device="cuda") * 0.3,
                           torch.tensor([f * hop for f in own_f], dtype=torch.int64, device="cuda")))

        def synth_loop():
            out = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.synthesize_device(model, hp, mels, S.device_batches(frames, cfg, hp), 75, True, lambda k, pcm: out.__setitem__(k, np.array(pcm)))
            return time.perf_counter() - t0, None

        def group_calls(sd):
            def run():
                def all_groups():
                    for gx, gy, gl in shapes:
                        sd.dist(gx, gy, lengths=gl)
                return timed(all_groups)
            return run
        legs += [("synth_loop", synth_loop), ("group_calls_1", group_calls(sd1)), ("group_calls_3", group_calls(sd3))]

    times, last = {name: [] for name, _ in legs}, {}
    for rnd in range(args.rounds + 1):                   # round 0 warms up and is not counted
        for name, fn in legs:
            dt, last[name] = fn()
            if rnd:
                times[name].append(dt)
            print("round %d %-14s %.6f s" % (rnd, name, dt), flush=True)

    def stats(ts):
        return {"s": statistics.median(ts), "s_min": min(ts), "s_max": max(ts), "rounds_s": [round(t, 7) for t in ts]}

    st = {k: stats(v) for k, v in times.items()}
    got1 = {k: v.cpu().numpy() for k, v in last["call_1"].items()}
    got3 = {k: v.cpu().numpy() for k, v in last["call_3"].items()}
    np1, np3 = last["numpy_1"], last["numpy_3"]
    tor3 = {k: v.cpu().numpy() for k, v in last["torch_3"].items()}

    def call_bytes(resolutions):
        n = 4 * M * (own[0] // 2 + 1) + 8 * M                 # the filterbank and bands, once
        for n_fft, h in resolutions + ([] if own in resolutions else [own]):
            parts = sum(-(-(1 + ln // h) // sd1._lib.fwn_spectral_distance_frames(n_fft, h)) for ln in lens)
            n += 2 * 4 * sum(lens) + 2 * 32 * parts + 32 * b + 8 * b
        return n

    def spectrogram_bytes(resolutions):                        # two complex64 spectrograms per resolution, written and read once
        return sum(2 * 2 * 8 * b * (1 + top // h) * (n_fft // 2 + 1) for n_fft, h in resolutions)

    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "frames_seed": FRAMES_SEED, "clips": b, "input_samples": sum(lens),
           "longest_clip": top, "mel_frames": sum(frames), "audio_seconds": sum(lens) / float(hp.sample_rate), "own_resolution": own,
           "three_resolutions": THREE,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "median of the rounds, the legs alternating within a round; "
                      "calls and the torch composition: HIP events; numpy and the synthesis loop: host wall clock"},
           "a_call": {"one_resolution": dict(st["call_1"], bytes_moved=call_bytes([own]),
                                             share_of_hbm_rate=call_bytes([own]) / st["call_1"]["s"] * 1e-9 / args.hbm_gbs),
                      "three_resolutions": dict(st["call_3"], bytes_moved=call_bytes(THREE),
                                                share_of_hbm_rate=call_bytes(THREE) / st["call_3"]["s"] * 1e-9 / args.hbm_gbs),
                      "hbm_rate_assumed_gb_per_s": args.hbm_gbs},
           "c_torch_composition": {"one_resolution": dict(st["torch_1"], spectrogram_bytes=spectrogram_bytes([own]),
                                                          times_the_call=st["torch_1"]["s"] / st["call_1"]["s"]),
                                   "three_resolutions": dict(st["torch_3"], spectrogram_bytes=spectrogram_bytes(THREE),
                                                             times_the_call=st["torch_3"]["s"] / st["call_3"]["s"]),
                                   "max_abs_diff_from_the_call_three_resolutions": {
                                       k: float(np.abs(tor3[k] - got3[k]).max()) for k in ("mel_l1", "lsd_db", "sc")}},
           "d_numpy_scipy_host": {"threads": args.threads, "one_resolution": dict(st["numpy_1"], times_the_call=st["numpy_1"]["s"] / st["call_1"]["s"]),
                                  "three_resolutions": dict(st["numpy_3"], times_the_call=st["numpy_3"]["s"] / st["call_3"]["s"]),
                                  "max_abs_diff_from_the_call": {
                                      "one_resolution": [float(np.abs(np1[:, i] - got1[k]).max()) for i, k in enumerate(("mel_l1", "lsd_db", "sc"))],
                                      "three_resolutions": [float(np.abs(np3[:, i] - got3[k]).max()) for i, k in enumerate(("mel_l1", "lsd_db", "sc"))]}},
           "means_over_the_clips": {k: float(got3[k].mean()) for k in ("mel_l1", "lsd_db", "sc")},
           "default_path": "NOT MEASURED by this tool: python bench.py on this commit against its parent"}
    if args.no_synth:
        res["b_share_of_the_synthesis_loop"] = "NOT MEASURED (--no_synth)"
    else:
        loop = st["synth_loop"]["s"]
        res["b_share_of_the_synthesis_loop"] = {
            "synthesize_device_rng_ragged_loop": st["synth_loop"], "calls": len(groups),
            "dist_over_the_groups_one_resolution": dict(st["group_calls_1"], share_of_the_loop=st["group_calls_1"]["s"] / loop),
            "dist_over_the_groups_three_resolutions": dict(st["group_calls_3"], share_of_the_loop=st["group_calls_3"]["s"] / loop)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["s"] for k, v in st.items()}))


if __name__ == "__main__":
    main()
