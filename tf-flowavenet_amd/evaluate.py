"""``evaluate`` CLI - how close synthesized audio is to its target: mel L1, log-spectral distance and spectral convergence
(``metrics.SpectralDistance``), one JSON line per utterance.  Two modes:

    python -m tf_flowavenet_amd.evaluate --saved_dir logs/pretrained/ --base_dir data/ --out eval.jsonl
        [--seed S] [--batch N] [--max_pad_frac f] [--denoise s] [--window W] [--resolutions 512/128,1024/256,2048/512]

copy-synthesis of a preprocessing output: ``train.txt`` is read as ``score`` reads it (the same ``read_metadata``, cropping and
``plan``), every ragged batch is synthesized from its stored mels with ``FloWaveNet.synthesize(..., lengths=, return_wav=True)``
- clip id = index in file order, so a clip's audio does not depend on its batch - and the float waveform (after ``Denoiser``
with ``--denoise``) is measured against the stored audio where it is, on the device.  Utterances longer than ``--window`` samples
go through ``synthesize_windowed(return_wav=True)``.

    python -m tf_flowavenet_amd.evaluate --ref_dir A --test_dir B --out eval.jsonl [--batch N] [--max_pad_frac f] [--resolutions ..]

two wav directories, no model: the ``*.wav`` of both are paired by name, read with ``load_wav`` at ``hparams.sample_rate`` (so
their rates may differ), each pair cropped to the shorter of the two, and the pairs batched by ``plan_batches``.  A name present
on one side only is listed in the summary; it is not an error.

Each line of ``--out``: ``{"name", "samples", "frames", "mel_l1", "lsd_db", "sc", "lsd_db@<n_fft>/<hop>", "sc@..."}`` in file
order (sorted names for directories); a measure that does not exist (a pair too short to frame, a silent target's ``sc``) is
``null``.  The last line, ``{"summary": true, ...}``, holds the plain means over the utterances that have the measure, in fp64
in file order, the counts, and the unpaired names.  Giving both modes, or neither whole, is a parser error.
"""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np

from .metrics import MEASURES, resolution_arg
from .score import plan, read_metadata, windowed_plan, cropped_frames
from .synthesize import plan_batches, window_samples


def eval_record(step, d, row=0):
    """``train.py --eval_metrics``: the record of ``<log_dir>/eval/summary.jsonl`` from ``SpectralDistance.dist``'s result."""
    rec = {"step": int(step)}
    for m in MEASURES:
        rec["eval/" + m] = float(d[m][row])
    return rec


def records_of(names, samples, d):
    """One record per row of ``d`` (name -> ``[B]`` array-likes on the host)."""
    out = []
    for row, (name, n) in enumerate(zip(names, samples)):
        rec = {"name": name, "samples": int(n), "frames": int(d["frames"][row])}
        for key in d:
            if key != "frames":
                v = float(d[key][row])
                rec[key] = v if math.isfinite(v) else None
        out.append(rec)
    return out


def summarize(records, extra=None):
    """The last line: the mean of every measure over the records that have it, summed in fp64 in order."""
    out = {"summary": True, "utterances": len(records)}
    keys = []
    for r in records:
        keys += [k for k in r if k not in ("name", "samples", "frames") and k not in keys]
    for k in keys:
        vals = [np.float64(r[k]) for r in records if r.get(k) is not None]
        s = np.float64(0.0)
        for v in vals:
            s = s + v
        out[k] = float(s / len(vals)) if vals else None
        out["measured/" + k] = len(vals)
    out.update(extra or {})
    return out


def write_out(path, records, summary):
    with open(path, "w", encoding="utf-8") as f:
        for r in records + [summary]:
            f.write(json.dumps(r) + "\n")


def _host(d):
    """The result dict -> host arrays: the one download of a batch."""
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in d.items()}


def pair_names(ref_dir, test_dir):
    """(paired, only in ref_dir, only in test_dir): ``*.wav`` names, each sorted."""
    ref = {f for f in os.listdir(ref_dir) if f.endswith(".wav")}
    test = {f for f in os.listdir(test_dir) if f.endswith(".wav")}
    return sorted(ref & test), sorted(ref - test), sorted(test - ref)


def _unmeasured(name, metric):
    rec = {"name": name, "samples": 0, "frames": 0, "mel_l1": None, "lsd_db": None, "sc": None}
    for n_fft, hop in metric.resolutions:
        rec["lsd_db@%d/%d" % (n_fft, hop)] = None
        rec["sc@%d/%d" % (n_fft, hop)] = None
    return rec


def evaluate_dirs(args, hparams, metric=None, device="cuda", load=None):
    """``--ref_dir / --test_dir``.  ``metric`` (default: a ``SpectralDistance``) and ``load`` (default ``load_wav``) are what a
    test replaces."""
    import torch
    from .preprocessing import load_wav
    if metric is None:
        from .metrics import SpectralDistance
        metric = SpectralDistance(hparams, getattr(args, "resolutions", None), device=device)
    load = load_wav if load is None else load
    names, only_ref, only_test = pair_names(args.ref_dir, args.test_dir)
    resamplers, clips = {}, []
    for n in names:
        a = load(os.path.join(args.ref_dir, n), hparams.sample_rate, resamplers)
        b = load(os.path.join(args.test_dir, n), hparams.sample_rate, resamplers)
        k = min(len(a), len(b))                      # cropped to the shorter of the two
        clips.append((np.asarray(a[:k], dtype=np.float32), np.asarray(b[:k], dtype=np.float32)))
    hop = hparams.hop_size
    live = [k for k, (a, _) in enumerate(clips) if len(a) > 0]
    records = {k: _unmeasured(names[k], metric) for k in range(len(names)) if k not in live}
    groups = plan_batches([-(-len(clips[k][0]) // hop) for k in live], int(args.batch), float(args.max_pad_frac), hparams)
    for group in groups:
        group = [live[g] for g in group]
        lens = [len(clips[k][0]) for k in group]
        x = np.zeros((len(group), max(lens)), dtype=np.float32)
        y = np.zeros_like(x)
        for row, k in enumerate(group):
            x[row, :lens[row]], y[row, :lens[row]] = clips[k]
        d = _host(metric.dist(torch.from_numpy(x).to(device), torch.from_numpy(y).to(device), lengths=lens))
        for k, rec in zip(group, records_of([names[k] for k in group], lens, d)):
            records[k] = rec
    out = [records[k] for k in sorted(records)]
    summary = summarize(out, {"only_in_ref_dir": only_ref, "only_in_test_dir": only_test})
    write_out(args.out, out, summary)
    return out, summary


def evaluate_synthesis(args, hparams, model=None, metric=None, device="cuda"):
    """Copy-synthesis of ``--base_dir`` with the model of ``--saved_dir``."""
    import torch
    from .synthesize import _denoiser, load_checkpoint
    if model is None:
        from .model import FloWaveNet
        model = FloWaveNet(hparams).load_params(load_checkpoint(args.saved_dir))
    if metric is None:
        from .metrics import SpectralDistance
        metric = SpectralDistance(hparams, getattr(args, "resolutions", None), device=device)
    denoiser = _denoiser(args, model)
    hop, seed = hparams.hop_size, int(args.seed)
    meta = read_metadata(args.base_dir)
    audios = [np.load(os.path.join(args.base_dir, "audios", a)).astype(np.float32).reshape(-1) for a, _ in meta]
    mels = [np.load(os.path.join(args.base_dir, "mels", m)).astype(np.float32) for _, m in meta]
    frames = [min(mel.shape[0], len(au) // hop) for au, mel in zip(audios, mels)]
    long_ones, planned, window = set(), frames, None
    if getattr(args, "window", None) is not None:
        window = window_samples(args.window, hparams)
        long_ones, planned = windowed_plan(frames, window, hparams)
    kept, groups = plan(planned, int(args.batch), float(args.max_pad_frac), hparams)
    for k in sorted(set(range(len(meta))) - set(kept) - long_ones):
        print("Skipping {}: {} frames are fewer than the model's alignment".format(meta[k][0], frames[k]))
    records = {}
    for k in sorted(long_ones):
        f = cropped_frames(frames[k], hparams)
        c = torch.from_numpy(mels[k][None, :f]).to(device)
        _, wav = model.synthesize_windowed(c, seed, clip_ids=[k], window=window, batch=int(args.batch), return_wav=True)
        y = wav[:, :, 0].contiguous()
        if denoiser is not None:
            y = denoiser(y)
        d = _host(metric.dist(torch.from_numpy(audios[k][None, :f * hop]).to(device), y))
        records[k] = records_of([meta[k][0]], [f * hop], d)[0]
    for group in groups:
        if all(kept[g] in long_ones for g in group):
            continue
        own = [cropped_frames(frames[kept[g]], hparams) for g in group]
        top, lens = max(own), [f * hop for f in own]
        x = np.zeros((len(group), top * hop), dtype=np.float32)
        c = np.zeros((len(group), top, hparams.num_mels), dtype=np.float32)
        for row, (g, f) in enumerate(zip(group, own)):
            x[row, :f * hop] = audios[kept[g]][:f * hop]
            c[row, :f] = mels[kept[g]][:f]
        _, wav = model.synthesize(torch.from_numpy(c).to(device), seed, clip_ids=[kept[g] for g in group], lengths=lens,
                                  return_wav=True)
        y = wav[:, :, 0].contiguous()
        if denoiser is not None:
            y = denoiser(y, lengths=lens)
        d = _host(metric.dist(torch.from_numpy(x).to(device), y, lengths=lens))
        for g, rec in zip(group, records_of([meta[kept[g]][0] for g in group], lens, d)):
            if kept[g] not in long_ones:
                records[kept[g]] = rec
    out = [records[k] for k in sorted(records)]
    summary = summarize(out)
    write_out(args.out, out, summary)
    return out, summary


def parse_args(argv=None):
    from .denoise import strength_arg

    def resolutions(text):
        try:
            return resolution_arg(text)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))

    parser = argparse.ArgumentParser(description="spectral distances of synthesized audio against its target")
    parser.add_argument("--saved_dir", default=None, help="copy-synthesis: folder with model checkpoint")
    parser.add_argument("--base_dir", default=None, help="copy-synthesis: preprocessing output (train.txt, audios/, mels/)")
    parser.add_argument("--ref_dir", default=None, help="two directories: the target wavs")
    parser.add_argument("--test_dir", default=None, help="two directories: the wavs under test, paired by name")
    parser.add_argument("--out", default="eval.jsonl", help="one JSON line per utterance and a summary line")
    parser.add_argument("--seed", type=int, default=1234, help="copy-synthesis: the latent's seed (clip id = index in train.txt)")
    parser.add_argument("--batch", type=int, default=8, help="utterances per launch (of similar length)")
    parser.add_argument("--max_pad_frac", type=float, default=0.25,
                        help="the largest share of a launch's samples that may be padding (synthesize.plan_batches)")
    parser.add_argument("--denoise", type=strength_arg, default=None, help="copy-synthesis: measure after Denoiser at this strength")
    parser.add_argument("--window", type=int, default=None,
                        help="copy-synthesis: utterances longer than this many samples are synthesized window by window")
    parser.add_argument("--resolutions", type=resolutions, default=None,
                        help="n_fft/hop[,n_fft/hop...] for lsd_db and sc (default: the model's own); mel_l1 is always the model's")
    args = parser.parse_args(argv)
    synth, dirs = (args.saved_dir, args.base_dir), (args.ref_dir, args.test_dir)
    if any(v is not None for v in synth) and any(v is not None for v in dirs):
        parser.error("give either --saved_dir/--base_dir (copy-synthesis) or --ref_dir/--test_dir (two directories), not both")
    if not (all(v is not None for v in synth) or all(v is not None for v in dirs)):
        parser.error("give --saved_dir and --base_dir, or --ref_dir and --test_dir")
    if args.ref_dir is not None and (args.denoise is not None or args.window is not None):
        parser.error("--denoise and --window belong to copy-synthesis")
    return args


def main(argv=None):
    from .hparams import hparams
    args = parse_args(argv)
    if args.ref_dir is not None:
        evaluate_dirs(args, hparams)
    else:
        evaluate_synthesis(args, hparams)


if __name__ == "__main__":
    main()
