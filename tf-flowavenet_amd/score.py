"""``score`` CLI - the likelihood of every utterance of a preprocessing output, one JSON line each:

    python -m tf_flowavenet_amd.score --saved_dir logs/pretrained/ --base_dir data/ --out scores.jsonl

``base_dir`` is what ``preprocessing`` writes: ``train.txt`` (``audio file|mel file|samples|...`` per line), ``audios/*.npy``
float32 [N * hop] and ``mels/*.npy`` float32 [N, num_mels].  Utterances of similar length share a call
(``synthesize.plan_batches`` with the same ``--batch`` / ``--max_pad_frac``) of ``FloWaveNet.forward(x, c, lengths=)``, which
gives every clip the ``log_p`` and ``logdet`` it gets alone.  An utterance is cropped to the model's alignment first: to the
largest number of frames whose samples divide by 2^n_block (model.py:226); one shorter than that is skipped with a message.

Each line of ``--out``: ``{"name": <audio file>, "samples": <samples scored>, "log_p": .., "logdet": .., "nll": -(log_p + logdet)}``
(nats per sample, train.py:56-60), in the order of ``train.txt``.

``--window SAMPLES`` (opt-in) scores every utterance longer than that through ``FloWaveNet.forward_windowed`` - window by
window with the network's receptive field of real context on both sides, the sums taken over the cores only - so no utterance
is too long for one call any more.  The other utterances keep their calls: the plan is made as without the flag (over
everything one call can address), a group of long utterances only is skipped, and a group that mixes both runs as it would
have - its short members' records are bit for bit those of a run without the flag, its long members' come from the windows.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .synthesize import load_checkpoint, max_clips_per_call, plan_batches, window_samples


def read_metadata(base_dir):
    """``train.txt`` -> [(audio file, mel file)] in file order."""
    out = []
    with open(os.path.join(base_dir, "train.txt"), encoding="utf-8") as f:
        for line in f:
            parts = line.rstrip("\n").split("|")
            if len(parts) >= 2 and parts[0]:
                out.append((parts[0], parts[1]))
    return out


def cropped_frames(frames, hparams):
    """The frames of an utterance that are scored: ``frames`` rounded DOWN so that frames * hop divides by 2^n_block."""
    align = max(1, (1 << hparams.n_block) // int(np.gcd(1 << hparams.n_block, hparams.hop_size)))
    return int(frames) - int(frames) % align


def plan(frame_counts, batch, max_pad_frac, hparams):
    """(kept, groups): the indices of the utterances long enough to score, and ``plan_batches`` groups of positions in
    ``kept``.  Pure host code."""
    kept = [k for k, f in enumerate(frame_counts) if cropped_frames(f, hparams) > 0]
    groups = plan_batches([cropped_frames(frame_counts[k], hparams) for k in kept], batch, max_pad_frac, hparams)
    return kept, groups


def windowed_plan(frame_counts, window, hparams):
    """``--window``: (long, planned) - the indices of the utterances whose cropped length exceeds ``window`` samples, and the
    frame counts the ordinary plan is made over: as given, but 0 for a long utterance that exceeds what one call can address
    (without the flag the plan would refuse it; every other utterance is planned as without the flag).  Pure host code."""
    hop = hparams.hop_size
    long_ones = {k for k, f in enumerate(frame_counts) if cropped_frames(f, hparams) * hop > int(window)}
    planned = [0 if k in long_ones and max_clips_per_call(hparams, cropped_frames(f, hparams) * hop) < 1 else f
               for k, f in enumerate(frame_counts)]
    return long_ones, planned


def score(args, hparams, model=None):
    import torch
    from .model import FloWaveNet
    if model is None:
        model = FloWaveNet(hparams).load_params(load_checkpoint(args.saved_dir))
    hop = hparams.hop_size
    meta = read_metadata(args.base_dir)
    audios = [np.load(os.path.join(args.base_dir, "audios", a)).astype(np.float32).reshape(-1) for a, _ in meta]
    mels = [np.load(os.path.join(args.base_dir, "mels", m)).astype(np.float32) for _, m in meta]
    frames = [min(mel.shape[0], len(au) // hop) for au, mel in zip(audios, mels)]
    # --window: the utterances longer than it are scored window by window; the plan is made over what it is made without the flag
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
        x = torch.from_numpy(audios[k][None, :f * hop, None]).cuda()
        c = torch.from_numpy(mels[k][None, :f]).cuda()
        log_p, logdet = model.forward_windowed(x, c, window=window, batch=int(args.batch))
        lp, ld = float(log_p[0]), float(logdet[0])
        records[k] = {"name": meta[k][0], "samples": f * hop, "log_p": lp, "logdet": ld, "nll": -(lp + ld)}
    for group in groups:
        if all(kept[g] in long_ones for g in group):
            continue                                 # (never without --window: long_ones is empty)
        own = [cropped_frames(frames[kept[g]], hparams) for g in group]
        top = max(own)
        x = np.zeros((len(group), top * hop, 1), dtype=np.float32)
        c = np.zeros((len(group), top, hparams.num_mels), dtype=np.float32)
        for row, (g, f) in enumerate(zip(group, own)):
            x[row, :f * hop, 0] = audios[kept[g]][:f * hop]
            c[row, :f] = mels[kept[g]][:f]
        log_p, logdet = model.forward(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda(), lengths=[f * hop for f in own])
        log_p, logdet = log_p.cpu().numpy(), logdet.cpu().numpy()
        for row, (g, f) in enumerate(zip(group, own)):
            if kept[g] in long_ones:
                continue                             # its record is the windowed one
            lp, ld = float(log_p[row]), float(logdet[row])
            records[kept[g]] = {"name": meta[kept[g]][0], "samples": f * hop, "log_p": lp, "logdet": ld, "nll": -(lp + ld)}
    out = [records[k] for k in sorted(records)]
    with open(args.out, "w", encoding="utf-8") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")
    return out


def main(argv=None):
    from .hparams import hparams
    parser = argparse.ArgumentParser()
    parser.add_argument("--saved_dir", default="logs/pretrained/", help="Folder with model checkpoint")
    parser.add_argument("--base_dir", default="./", help="preprocessing output: train.txt, audios/, mels/")
    parser.add_argument("--out", default="scores.jsonl", help="one JSON line per utterance")
    parser.add_argument("--batch", type=int, default=8, help="utterances per launch (of similar length)")
    parser.add_argument("--max_pad_frac", type=float, default=0.25,
                        help="the largest share of a launch's samples that may be padding (synthesize.plan_batches)")
    # absent from the namespace unless given: without the flag nothing changes
    parser.add_argument("--window", type=int, default=argparse.SUPPRESS,
                        help="score utterances longer than this many samples window by window (FloWaveNet.forward_windowed)")
    args = parser.parse_args(argv)
    score(args, hparams)


if __name__ == "__main__":
    main()
