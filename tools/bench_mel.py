"""The ragged mel front-end on one MI355X:

    python tools/bench_mel.py --out profiles/mel_frontend.json

over the 64 utterances of 200 - 900 mel frames of ``tools/bench_synth.py`` (``FRAMES``; seeded noise of the clips' lengths, float32
on the host, as ``load_wav`` hands them over):

  (a) the per-clip way: ``_process_utterance`` per clip with one ``MelSpectrogram`` (host peak and padding, one upload, one
      ``fwn_mel_spectrogram`` launch and one download per clip), host wall clock;
  (b) one ``MelFrontEnd`` call over all clips - one upload, two launches, one download of audio, mel and peak -, host wall clock;
  (c) the two launches of (b) alone, by device events around each: time, the bytes each has to move (every clip's own samples in;
      the peaks, and every row of mel and audio, out; the filterbank once) and that as a share of the HBM rate given by
      ``--hbm_gbs``;
  (d) ``mel_kernel`` (``fwn_mel_spectrogram``, the direct DFT) against ``mel_front_kernel`` alone (no normalisation, no audio) on
      one rectangular batch of the same number of frames, by device events;
  (e) is not this tool's: the default path is ``python bench.py`` on this commit against its parent, alternating on one box.

One untimed round first, then ``--rounds`` rounds that run the legs one after the other (alternating them: other people's work
shares the host); a figure is the median of its rounds.  Reads nothing outside the repository.  A run without a GPU fails."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=len(FRAMES), help="use the first N utterances only (rehearsals)")
    ap.add_argument("--hbm_gbs", type=float, default=8000.0, help="the HBM rate the share is taken of (MI355X data sheet: 8 TB/s)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel.py measures on the GPU: none found")
    from tf_flowavenet_amd import preprocessing as P
    from tf_flowavenet_amd.hparams import default_hparams
    hp = default_hparams()
    hop, n_fft, M = hp.hop_size, hp.n_fft, hp.num_mels
    rng = np.random.default_rng(FRAMES_SEED)
    # f frames <-> f * hop - 1 samples (1 + N div hop = f), so the clips' frame counts are FRAMES
    lens = [f * hop - 1 for f in FRAMES[:args.clips]]
    clips = [np.clip(rng.normal(0.0, 0.3, n), -1.0, 1.0).astype(np.float32) for n in lens]
    top = max(lens)
    frames = [1 + n // hop for n in lens]
    f_host = 1 + top // hop
    mel_fn, front = P.MelSpectrogram(hp), P.MelFrontEnd(hp)

    def per_clip():
        t0 = time.perf_counter()
        out = [P._process_utterance(c, hp, mel_fn) for c in clips]
        return time.perf_counter() - t0, out

    def one_call():
        t0 = time.perf_counter()
        x, _ = P.ragged_rows(clips, "cuda")
        audio, mel, peak = front(x, lengths=lens)
        flat = torch.cat([audio.reshape(-1), mel.reshape(-1), peak]).cpu().numpy()
        return time.perf_counter() - t0, flat

    x_dev, _ = P.ragged_rows(clips, "cuda")
    lens_dev = torch.tensor(lens, dtype=torch.int64).cuda()
    lib, stream = front._lib, torch.cuda.current_stream().cuda_stream
    peak = torch.empty(len(lens), device="cuda")
    mel = torch.empty(len(lens), f_host, M, device="cuda")
    audio = torch.empty(len(lens), f_host * hop, device="cuda")

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    def launch_peak():
        return timed(lambda: lib.fwn_clip_peak(x_dev.data_ptr(), len(lens), top, lens_dev.data_ptr(), top, peak.data_ptr(), stream)), None

    def launch_front():
        return timed(lambda: lib.fwn_mel_front(x_dev.data_ptr(), len(lens), top, lens_dev.data_ptr(), top, peak.data_ptr(),
                                               float(hp.rescaling_max), front._fb.data_ptr(), front._bands.data_ptr(), n_fft, hop, M,
                                               float(hp.ref_level_db), float(hp.min_level_db), mel.data_ptr(), f_host * M,
                                               audio.data_ptr(), f_host * hop, stream)), None

    # (d): a rectangle of about the same number of frames: 64 rows of the mean length
    rect_t = (sum(frames) // len(frames)) * hop - 1
    rect = torch.from_numpy(np.clip(rng.normal(0.0, 0.3, (len(lens), rect_t)), -1.0, 1.0).astype(np.float32)).cuda()
    rect_frames = len(lens) * (1 + rect_t // hop)
    rect_mel = torch.empty(len(lens), 1 + rect_t // hop, M, device="cuda")
    rect_mel2 = torch.empty_like(rect_mel)

    def dft_kernel():
        return timed(lambda: lib.fwn_mel_spectrogram(rect.data_ptr(), len(lens), rect_t, mel_fn._win.data_ptr(), mel_fn._fb.data_ptr(), n_fft,
                                                     hop, M, float(hp.ref_level_db), float(hp.min_level_db), rect_mel.data_ptr(), stream)), None

    def fft_kernel():
        return timed(lambda: lib.fwn_mel_front(rect.data_ptr(), len(lens), rect_t, None, rect_t, None, 1.0, front._fb.data_ptr(),
                                               front._bands.data_ptr(), n_fft, hop, M, float(hp.ref_level_db), float(hp.min_level_db),
                                               rect_mel2.data_ptr(), rect_mel2[0].numel(), None, 0, stream)), None

    legs = [("per_clip", per_clip), ("one_call", one_call), ("peak_launch", launch_peak), ("front_launch", launch_front),
            ("dft_kernel", dft_kernel), ("fft_kernel", fft_kernel)]
    times, last = {name: [] for name, _ in legs}, {}
    for rnd in range(args.rounds + 1):                   # round 0 warms up and is not counted
        for name, fn in legs:
            dt, last[name] = fn()
            if rnd:
                times[name].append(dt)
            print("round %d %-14s %.6f s" % (rnd, name, dt), flush=True)

    # the legs computed the same thing: audio bit for bit, mels to the suite's tolerance (DFT against FFT)
    flat = last["one_call"]
    b, na, nm = len(lens), f_host * hop, f_host * M
    a1, m1 = flat[:b * na].reshape(b, na), flat[b * na:b * (na + nm)].reshape(b, f_host, M)
    audio_equal = all(np.array_equal(a1[k, :frames[k] * hop], last["per_clip"][k][0]) for k in range(b))
    mel_diff = max(float(np.abs(m1[k, :frames[k]] - last["per_clip"][k][1]).max()) for k in range(b))
    rect_diff = float((rect_mel - rect_mel2).abs().max())

    def stats(ts):
        return {"s": statistics.median(ts), "s_min": min(ts), "s_max": max(ts), "rounds_s": [round(t, 7) for t in ts]}

    st = {k: stats(v) for k, v in times.items()}
    audio_s = sum(lens) / float(hp.sample_rate)
    peak_bytes = 4 * sum(lens) + 4 * b
    front_bytes = 4 * sum(lens) + 4 * b * (nm + na) + 4 * front._fb.numel() + 4 * b
    res = {"label": args.label, "gpu": torch.cuda.get_device_name(0), "frames_seed": FRAMES_SEED, "clips": b, "n_fft": n_fft, "hop": hop,
           "num_mels": M, "input_samples": sum(lens), "longest_clip": top, "mel_frames": sum(frames), "audio_seconds": audio_s,
           "frames_per_workgroup": front.frames_per_workgroup,
           "timing": {"rounds": args.rounds, "warmup_rounds": 1, "clock": "median of the rounds, the legs alternating within a round; "
                      "per_clip and one_call: host wall clock, uploads and downloads included; the launches and kernels: HIP events"},
           "a_per_clip_process_utterance": dict(st["per_clip"], ms_per_utterance=1e3 * st["per_clip"]["s"] / b),
           "b_one_mel_front_end_call": dict(st["one_call"], ms_per_utterance=1e3 * st["one_call"]["s"] / b,
                                            speedup_over_per_clip=st["per_clip"]["s"] / st["one_call"]["s"],
                                            audio_bit_equal_to_per_clip=bool(audio_equal), max_mel_diff_from_per_clip=mel_diff),
           "c_launches": {"fwn_clip_peak": dict(st["peak_launch"], bytes_moved=peak_bytes, gb_per_s=peak_bytes / st["peak_launch"]["s"] * 1e-9,
                                                share_of_hbm_rate=peak_bytes / st["peak_launch"]["s"] * 1e-9 / args.hbm_gbs),
                          "fwn_mel_front": dict(st["front_launch"], bytes_moved=front_bytes, gb_per_s=front_bytes / st["front_launch"]["s"] * 1e-9,
                                                share_of_hbm_rate=front_bytes / st["front_launch"]["s"] * 1e-9 / args.hbm_gbs,
                                                frames_per_s=sum(frames) / st["front_launch"]["s"]),
                          "hbm_rate_assumed_gb_per_s": args.hbm_gbs},
           "d_kernels_on_a_rectangle": {"rows": b, "samples_per_row": rect_t, "frames": rect_frames, "mel_kernel_dft": st["dft_kernel"],
                                        "mel_front_kernel_fft": st["fft_kernel"], "fft_speedup": st["dft_kernel"]["s"] / st["fft_kernel"]["s"],
                                        "max_mel_diff": rect_diff},
           "default_path": "NOT MEASURED by this tool: python bench.py on this commit against its parent"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"per_clip_s": st["per_clip"]["s"], "one_call_s": st["one_call"]["s"], "peak_launch_s": st["peak_launch"]["s"],
                      "front_launch_s": st["front_launch"]["s"], "dft_kernel_s": st["dft_kernel"]["s"], "fft_kernel_s": st["fft_kernel"]["s"],
                      "audio_bit_equal": bool(audio_equal), "max_mel_diff": mel_diff, "rect_max_mel_diff": rect_diff}))


if __name__ == "__main__":
    main()
