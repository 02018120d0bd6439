"""``train`` CLI - the reference's training loop (train.py:153-283) on MI355X.

    python -m tf_flowavenet_amd.train --base_dir data/ --input training_data/train.txt
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m tf_flowavenet_amd.train --base_dir data/            # one process per GPU, RCCL gradient all-reduce

Same flags as the reference (``--base_dir --input --restore --summary_interval --checkpoint_interval
--eval_interval --train_steps``) plus ``--log_dir`` / ``--seed`` / ``--ragged`` / ``--ragged_init``.  Input is the output of
``preprocessing.preprocess``: ``train.txt`` with ``audios/*.npy`` and ``mels/*.npy`` beside it.

Differences (deliberate): the TFRecord round trip (tfrecord.py, dataset.py:20-44) is skipped - the
``.npy`` files are read directly and cropped like ``Dataset._load_sample`` (dataset.py:70-76)
(``--input training_data/train.tfrecord`` reads the reference's TFRecords instead, ``tfrecord.py``); the
train / test split is the reference's ``train_test_split(test_size, random_state)`` (tfrecord.py:81-82);
summaries are JSON lines (``<log_dir>/train/summary.jsonl``, ``test/summary.jsonl``) and evaluation
audio is written as wav files instead of TensorBoard events; checkpoints are ``.npz`` files that
``synthesize.py`` loads (parameters in the reference's layouts, plus the Adam slots and global step).

``--ragged``: utterances shorter than ``max_time_steps`` train too.  Every utterance of at least lcm(hop_size, 2^n_block)
samples is kept; longer ones are cropped to ``max_time_steps`` at a random start as before, shorter ones go in whole (floored
to that unit) with their length, and the step takes the lengths (``Trainer.step(x, c, lengths=)``: loss and gradients are means
over the clips of each clip's own, padding reaches neither).  The batch shape stays ``max_time_steps``, so the step is recorded
once.  The held-out loss follows the same rule (per-clip ``log_p`` / ``logdet``, what ``score`` reports per utterance); the
data-dependent init batch is drawn from full-length crops (``Dataset.next_full``) wherever the corpus has an utterance longer
than ``max_time_steps``; where it has none - prompts, commands, digits - the init takes a ragged batch drawn like a training
batch (``Dataset.next_init``, ``Trainer.ddi(x, c, lengths=)``: ActNorm statistics over the clips' own samples), and the
init-step update runs with those lengths.  ``--ragged_init`` takes the ragged init batch on any corpus.

``--device_corpus``: the eligible training utterances are uploaded once (``corpus.DeviceCorpus``: audio and mels back to back and
a table of frame offsets) and every training batch is drawn and gathered there by ``fwn_corpus_draw`` on the training stream -
the same eligibility, crop range and short-utterance rule as ``Dataset``, but a Philox stream of this project's own keyed by
(seed, rank, draw counter), so the batches are not those of a run without the flag.  The counter lives on the device, moves by
one per draw, and goes into every checkpoint as ``__data/draw_counter``: a restored run continues the data stream where it
stopped (the host ``Dataset`` of a run without the flag starts its draws over).  The init batch, the held-out loss and the
evaluation sample stay with the host ``Dataset``.  Every rank of a data-parallel run holds the whole corpus.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import collections
import time

import numpy as np


class Dataset:
    """Random fixed-length crops of (mel, audio) pairs (dataset.py:47-85).

    ragged: utterances of at least lcm(hop_size, 2^n_block) samples are kept; one longer than ``max_time_steps`` is cropped as
    before, a shorter one goes in whole, floored to that unit and zero-padded to ``max_time_steps``; ``next_train`` /
    ``next_test`` then return ``(mels, audios, lengths)`` with ``lengths`` the clips' sample counts (int32 [B])."""
    # memory-mapped utterances kept open per rank (_load).  Every numpy memmap pins a dup'd file descriptor, two per
    # utterance: 64 pairs = 128 descriptors, far below the usual soft RLIMIT_NOFILE of 1024 that the GPU runtime, RCCL
    # and the log files also draw on.
    MAX_OPEN = 64

    def __init__(self, metadata_path, hparams, seed=None, rank=0, ragged=False):
        self._hp = hparams
        self._ragged = bool(ragged)
        self._basedir = os.path.dirname(metadata_path)
        with open(metadata_path, "rt", encoding="utf-8") as f:
            meta = [m.split("|") for m in f.read().strip().split("\n") if m]
        self._frames = hparams.max_time_steps // hparams.hop_size            # dataset.py:13-14
        self._steps = self._frames * hparams.hop_size
        # dataset.py:73 draws the crop start from [0, frames - max_time_frames): needs strictly longer clips
        if self._ragged:
            meta = [m for m in meta if int(m[2]) // hparams.hop_size >= self._unit_frames()]
            if not meta:
                raise ValueError("no utterance of at least lcm(hop_size, 2^n_block)=%d samples in %s"
                                 % (self._unit_frames() * hparams.hop_size, metadata_path))
        else:
            meta = [m for m in meta if int(m[2]) // hparams.hop_size > self._frames]
            if not meta:
                raise ValueError("no utterance longer than max_time_steps=%d in %s" % (hparams.max_time_steps, metadata_path))
        idx = np.arange(len(meta))
        if len(meta) > hparams.test_size:                                    # tfrecord.py:81-82
            from sklearn.model_selection import train_test_split
            tr, te = train_test_split(idx, test_size=hparams.test_size, random_state=hparams.split_random_state)
        else:
            tr, te = idx, idx
        self.train_meta, self.test_meta = [meta[i] for i in tr], [meta[i] for i in te]
        base = hparams.shuffle_random_seed if seed is None else seed
        self._rng = np.random.RandomState(base + 7919 * rank)
        self._cache, self._lru = {}, collections.OrderedDict()

    def _unit_frames(self):
        """lcm(hop_size, 2^n_block) in frames: the unit a ragged clip's length is a multiple of."""
        import math
        return math.lcm(self._hp.hop_size, 1 << self._hp.n_block) // self._hp.hop_size

    @classmethod
    def from_tfrecords(cls, train_path, test_path, hparams, seed=None, rank=0, ragged=False):
        """The reference's own data files (tfrecord.py:76-88): ``train.tfrecord`` / ``test.tfrecord``."""
        from . import tfrecord
        self = cls.__new__(cls)
        self._hp, self._basedir = hparams, os.path.dirname(train_path)
        self._ragged = bool(ragged)
        self._frames = hparams.max_time_steps // hparams.hop_size
        self._steps = self._frames * hparams.hop_size
        self._cache, self._lru = {}, collections.OrderedDict()      # TFRecord samples stay resident (not in the LRU)

        def load(path, tag):
            metas = []
            for k, (audio, mel, spk) in enumerate(tfrecord.read_samples(path)):
                if mel.shape[0] >= self._unit_frames() if self._ragged else mel.shape[0] > self._frames:
                    key = "%s-%d" % (tag, k)
                    self._cache[key] = (audio, mel)
                    metas.append([key, key, str(len(audio)), str(spk), ""])
            return metas

        self.train_meta = load(train_path, "train")
        self.test_meta = load(test_path, "test") if test_path and os.path.exists(test_path) else self.train_meta
        if not self.train_meta:
            raise ValueError(("no utterance of at least lcm(hop_size, 2^n_block) samples in %s" % train_path) if self._ragged else
                             "no utterance longer than max_time_steps=%d in %s" % (hparams.max_time_steps, train_path))
        base = hparams.shuffle_random_seed if seed is None else seed
        self._rng = np.random.RandomState(base + 7919 * rank)
        return self

    def _load(self, m):
        """Utterances read from ``audios/`` / ``mels/`` are memory-mapped (a crop touches a few pages; nothing of an
        LJSpeech-sized set stays resident per rank), with at most ``MAX_OPEN`` maps kept open (LRU)."""
        hit = self._cache.get(m[0])
        if hit is not None:
            if m[0] in self._lru:
                self._lru.move_to_end(m[0])
            return hit
        pair = (np.load(os.path.join(self._basedir, "audios", m[0]), mmap_mode="r"),
                np.load(os.path.join(self._basedir, "mels", m[1]), mmap_mode="r"))
        self._cache[m[0]] = pair
        self._lru[m[0]] = None
        while len(self._lru) > self.MAX_OPEN:
            old, _ = self._lru.popitem(last=False)
            # Dropping the pair releases the descriptors: a np.memmap holds a buffer export on its mmap object (an explicit
            # mmap.close() raises BufferError while the array exists), so the map and its file descriptor go when CPython
            # drops the LAST reference to the arrays - here, unless a caller kept a view.  _batch() copies its crops out
            # (np.empty + slice assignment) and keeps none; tests/test_train_cli.py bounds the open descriptors.
            del self._cache[old]
        return pair

    def _batch(self, metas):
        hp = self._hp
        ragged = self._ragged
        mels = (np.zeros if ragged else np.empty)((len(metas), self._frames, hp.num_mels), dtype=np.float32)
        audios = (np.zeros if ragged else np.empty)((len(metas), self._steps), dtype=np.float32)
        lengths = np.full(len(metas), self._steps, dtype=np.int32)
        for k, m in enumerate(metas):
            audio, mel = self._load(m)
            if ragged and mel.shape[0] <= self._frames:                      # a short utterance: whole, floored to the unit
                u = self._unit_frames()
                frames = min(mel.shape[0], len(audio) // hp.hop_size) // u * u
                mels[k, :frames] = mel[:frames]
                audios[k, :frames * hp.hop_size] = audio[:frames * hp.hop_size]
                lengths[k] = frames * hp.hop_size
            else:
                start = self._rng.randint(0, mel.shape[0] - self._frames)    # dataset.py:73-76
                mels[k] = mel[start:start + self._frames]
                audios[k] = audio[start * hp.hop_size:start * hp.hop_size + self._steps]
            del audio, mel              # the batch holds copies: no view outlives this iteration (see _load's close)
        return (mels, audios, lengths) if ragged else (mels, audios)

    def next_train(self):
        pick = self._rng.randint(0, len(self.train_meta), size=self._hp.batch_size)
        return self._batch([self.train_meta[i] for i in pick])

    def next_full(self):
        """A batch of full-length crops ``(mels, audios)`` whatever the mode: the data-dependent init takes no lengths."""
        full = [m for m in self.train_meta if int(m[2]) // self._hp.hop_size > self._frames]
        if not full:
            raise ValueError("--ragged: the ActNorm data-dependent init needs a batch of full-length crops (init=True takes no "
                             "lengths), and no training utterance is longer than max_time_steps=%d" % self._hp.max_time_steps)
        pick = self._rng.randint(0, len(full), size=self._hp.batch_size)
        return self._batch([full[i] for i in pick])[:2]

    def has_full(self):
        """Whether ``next_full`` has anything to draw from: a training utterance longer than ``max_time_steps``."""
        return any(int(m[2]) // self._hp.hop_size > self._frames for m in self.train_meta)

    def next_init(self):
        """The batch of a data-dependent init that takes lengths, drawn as ``next_train`` draws: ``(mels, audios, lengths)`` in
        ragged mode, ``next_train``'s pair otherwise."""
        return self.next_train()

    def next_test(self):
        pick = self._rng.randint(0, len(self.test_meta), size=self._hp.batch_size)
        return self._batch([self.test_meta[i] for i in pick])

    def eval_sample(self):
        """One utterance, capped at eval_max_time_steps (train.py:118-131)."""
        hp = self._hp
        m = self.test_meta[self._rng.randint(0, len(self.test_meta))]
        audio, mel = self._load(m)
        frames = min(int(hp.eval_max_time_steps // hp.hop_size), mel.shape[0])
        while frames > 1 and (frames * hp.hop_size) % (1 << hp.n_block):      # model.py:226: T % 2^n_block == 0
            frames -= 1
        return np.array(mel[:frames]), np.array(audio[:frames * hp.hop_size])   # copies, not views of the map


def save_checkpoint(path, trainer, corpus=None):
    """corpus: a ``corpus.DeviceCorpus`` - its draw counter goes in as ``__data/draw_counter`` (uint64), so that a restored run
    continues the data stream where this one stopped."""
    views = trainer.opt.master_views()
    out = {k: v.detach().cpu().numpy() for k, v in views.items()}
    if corpus is not None:
        out[DRAW_COUNTER_KEY] = np.asarray(corpus.counter, dtype=np.uint64)
    out["__opt/m"] = trainer.opt.m.cpu().numpy()
    out["__opt/v"] = trainer.opt.v.cpu().numpy()
    out["__opt/global_step"] = np.asarray(trainer.opt.global_step, dtype=np.int64)
    tmp = path + ".tmp"              # outside every restore glob (*.npz): a crash mid-write never shadows a good checkpoint
    with open(tmp, "wb") as f:
        np.savez(f, **out)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


DRAW_COUNTER_KEY = "__data/draw_counter"      # optional: written and read with --device_corpus only


def checkpoint_files(save_dir):
    """``flowavenet_model.ckpt-<step>.npz`` files of save_dir, oldest step first (by step number, not mtime)."""
    import re
    found = []
    for path in glob.glob(os.path.join(save_dir, "flowavenet_model.ckpt-*.npz")):
        m = re.search(r"ckpt-(\d+)\.npz$", path)
        if m:
            found.append((int(m.group(1)), path))
    return [p for _, p in sorted(found)]


def _checkpoint_step(path):
    import re
    return int(re.search(r"ckpt-(\d+)\.npz$", path).group(1))


def restore_checkpoint(save_dir, trainer, corpus=None):
    """Highest-step readable ``flowavenet_model.ckpt-<step>.npz`` -> masters, Adam slots, global step.  Returns the
    step or None.  corpus: a ``corpus.DeviceCorpus`` - its draw counter is set from ``__data/draw_counter`` where the file has
    one (a checkpoint written without ``--device_corpus`` has none: the counter stays); without a corpus the entry is ignored.

    Only a file that cannot be READ (truncated by a crash: zip / EOF / OS errors) is skipped, with a message.  A file
    that reads but does not fit this model - a missing parameter, another shape: different hparams - raises: silently
    starting from step 0 would go on to overwrite the run's checkpoints.  In a data-parallel job rank 0 picks the file
    and every rank must load that very step; disagreement (a file one rank cannot read) aborts the job."""
    import zipfile
    import torch
    import torch.distributed as dist
    group = getattr(trainer.opt, "group", None)
    multi = dist.is_available() and dist.is_initialized() and group is not False and dist.get_world_size(group) > 1
    files = list(reversed(checkpoint_files(save_dir)))
    want = None
    if multi:      # the step rank 0 is about to try first; ranks that see other files fail below instead of diverging
        box = [(_checkpoint_step(files[0]) if files else -1) if dist.get_rank(group) == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        want = box[0]
    got = None
    for path in files:
        if want is not None and got is None and _checkpoint_step(path) > want >= 0:
            continue                    # newer than what rank 0 sees (it is still being written there)
        try:
            with np.load(path) as f:
                names = set(f.files)
                arrays = {k: f[k] for k in names}
        except (zipfile.BadZipFile, EOFError, OSError, ValueError) as e:      # I/O and container-format errors only
            print("Skipping unreadable checkpoint {} ({}: {})".format(path, type(e).__name__, e))
            continue                    # (data parallel: if only this rank cannot read it, the agreement check below aborts)
        views = trainer.opt.master_views()
        missing = [k for k in list(views) + ["__opt/m", "__opt/v", "__opt/global_step"] if k not in names]
        if missing:
            raise KeyError("checkpoint {} does not belong to this model: {} entries missing, e.g. {!r} (other hparams?)"
                           .format(path, len(missing), missing[0]))
        for k, v in views.items():
            if int(np.prod(arrays[k].shape)) != v.numel():
                raise ValueError("checkpoint {}: {!r} has shape {}, the model expects {} (other hparams?)"
                                 .format(path, k, tuple(arrays[k].shape), tuple(v.shape)))
        loaded = {k: torch.from_numpy(arrays[k]).reshape(v.shape) for k, v in views.items()}
        m, v_, gs = torch.from_numpy(arrays["__opt/m"]), torch.from_numpy(arrays["__opt/v"]), int(arrays["__opt/global_step"])
        if m.numel() != trainer.opt.m.numel() or v_.numel() != trainer.opt.v.numel():
            raise ValueError("checkpoint {}: Adam slots of {} elements, the model has {}".format(path, m.numel(), trainer.opt.m.numel()))
        got = (path, loaded, m, v_, gs, int(arrays[DRAW_COUNTER_KEY]) if DRAW_COUNTER_KEY in names else None)
        break
    if multi:
        mine = torch.tensor([got[4] if got else -1], dtype=torch.int64, device=trainer.opt.m.device)
        lo, hi = mine.clone(), mine.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
        if int(lo) != int(hi):
            raise RuntimeError("ranks disagree on the checkpoint to restore (steps {} .. {}; this rank: {}): every rank "
                               "must read the same file of {}".format(int(lo), int(hi), int(mine), save_dir))
    if got is not None:
        path, loaded, m, v_, gs, draws = got
        views = trainer.opt.master_views()
        print("Loading checkpoint {}".format(path))
        if corpus is not None and draws is not None:
            corpus.set_counter(draws)
        for k, v in views.items():
            v.copy_(loaded[k])
        trainer.opt.m.copy_(m)
        trainer.opt.v.copy_(v_)
        trainer.opt.global_step = gs
        return gs
    return None


def train(log_dir, args, hparams, input_path, device="cuda", params=None):
    import torch
    import torch.distributed as dist
    from . import weights
    from .model import FloWaveNet
    from .optim import learning_rate
    from .synthesize import write_wav
    from .training import Trainer

    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    save_dir = os.path.join(log_dir, "pretrained")
    train_logdir, test_logdir = os.path.join(log_dir, "train"), os.path.join(log_dir, "test")
    for d in (save_dir, train_logdir, test_logdir):
        os.makedirs(d, exist_ok=True)
    checkpoint_path = os.path.join(save_dir, "flowavenet_model.ckpt")
    metadata_filename = os.path.join(args.base_dir, input_path)
    if rank == 0:
        print("Checkpoint_path: {}".format(checkpoint_path))
        print("Loading training data from: {}".format(metadata_filename))
    seed = getattr(args, "seed", None)
    ragged = bool(getattr(args, "ragged", False))
    if metadata_filename.endswith(".tfrecord"):       # the reference's own files (train.py:161-162)
        dataset = Dataset.from_tfrecords(metadata_filename, os.path.join(os.path.dirname(metadata_filename), "test.tfrecord"),
                                         hparams, seed=seed, rank=rank, ragged=ragged)
    else:
        dataset = Dataset(metadata_filename, hparams, seed=seed, rank=rank, ragged=ragged)
    if params is None:     # the reference's initialisers: he-uniform convs, g = 1, ZeroConv1d all zeros (modules.py:21-22,47-49)
        params = weights.synthetic_params(hparams, hparams.tf_random_seed if seed is None else seed, zero_conv="zeros")
    trainer = Trainer(hparams, params, device=device)
    # --device_corpus: the training split goes to the device once and every training batch is drawn there (corpus.py); the
    # init batch, the held-out loss and the evaluation sample stay with the host Dataset
    corpus = None
    if bool(getattr(args, "device_corpus", False)):
        from .corpus import DeviceCorpus
        corpus = DeviceCorpus(dataset, hparams, seed=seed, rank=rank, device=device)
    step = None
    if args.restore:
        step = restore_checkpoint(save_dir, trainer, corpus)
    if step is None:
        if rank == 0:
            print("Starting new training!" if not args.restore else "No checkpoint found.")
            print("Init ActNorm layer...", end="")
        # --ragged: full-length crops where the corpus has any (no lengths); a ragged batch where it has none, or on request
        lens = None
        if ragged and (bool(getattr(args, "ragged_init", False)) or not dataset.has_full()):
            mels, audios, lens = dataset.next_init()
        else:
            mels, audios = dataset.next_full() if ragged else dataset.next_train()
        trainer.ddi(audios, mels, lengths=lens)                               # train.py:221,229 (init=True)
        init_loss = float(trainer.step(audios, mels, lengths=lens)[0])       # ... which also applies an update
        step = trainer.opt.global_step
        if rank == 0:
            print(" OK. Init loss: {:.5f}".format(init_loss))
    if rank == 0:
        print("FloWaveNet training set to a maximum of {} steps".format(args.train_steps))

    def log(path, rec):
        with open(os.path.join(path, "summary.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")

    # --accum_steps K: an update is K draws, K - 1 through accumulate and the last through step, in draw order; every rank runs
    # this very loop, so all of them accumulate the same number of times per update.  Steps, the rate schedule and every
    # interval below count updates, and a checkpoint is only ever written between two updates: no pending state to save.
    accum_steps = int(getattr(args, "accum_steps", 1))
    eval_metric = None                                                       # --eval_metrics: built at the first evaluation
    while step < args.train_steps:
        start_time = time.time()
        clip_lengths = []
        # (device corpus: the lengths are on the device; they are kept - a clone per micro-batch, no read - only for an update
        # that writes a summary)
        keep_lengths = ragged and rank == 0 and (step + 1) % args.summary_interval == 0
        for micro in range(accum_steps):
            run = trainer.step if micro == accum_steps - 1 else trainer.accumulate
            if corpus is not None:
                audios, mels, lens = corpus.draw(hparams.batch_size)
                out = run(audios, mels, lengths=lens)
                if keep_lengths:
                    clip_lengths.append(lens.tensor.clone())
            elif ragged:
                mels, audios, lens = dataset.next_train()
                out = run(audios, mels, lengths=lens)
                clip_lengths.extend(lens)
            else:
                mels, audios = dataset.next_train()
                out = run(audios, mels)
        loss, log_p, logdet, gnorm = out
        step = trainer.opt.global_step
        total_loss = float(loss)                                             # synchronises: the step time is real
        step_duration = time.time() - start_time
        if rank == 0:
            print("Step {:7d} [{:.3f} sec/step, loss={:.5f}, log_p={:.5f}, logdet={:.5f}]".format(
                step, step_duration, total_loss, float(log_p), float(logdet)), end="\r")
        if rank == 0 and step % args.summary_interval == 0:
            print("\nWriting summary at step {}".format(step))
            rec = {"step": step, "losses/total_loss": total_loss, "losses/log_p": float(log_p),
                   "losses/logdet": float(logdet), "learning_rate": learning_rate(step - 1),
                   "gradient_global_norm": float(gnorm), "accum_steps": accum_steps}
            if ragged:
                if corpus is not None:
                    clip_lengths = torch.cat(clip_lengths).cpu().numpy()
                rec["mean_clip_length"] = float(np.mean(clip_lengths))
            log(train_logdir, rec)
            model = FloWaveNet(hparams, device=device, cond_mode=1).load_params(trainer.opt.master_views())
            if ragged:      # per-clip scalars, each over the clip's own samples: the numbers `score` reports per utterance
                tm, ta, tl = dataset.next_test()
                tlp, tld = model.forward(torch.from_numpy(ta).reshape(ta.shape[0], -1, 1), torch.from_numpy(tm), lengths=tl)
                tlp, tld = tlp.double().mean(), tld.double().mean()
            else:
                tm, ta = dataset.next_test()                                 # get_test_losses, train.py:85-91
                tlp, tld = model.forward(torch.from_numpy(ta).reshape(ta.shape[0], -1, 1), torch.from_numpy(tm))
            rec = {"step": step, "losses/total_loss": -(float(tlp) + float(tld)),
                   "losses/log_p": float(tlp), "losses/logdet": float(tld)}
            if ragged:
                rec["mean_clip_length"] = float(np.mean(tl))
            log(test_logdir, rec)
        if rank == 0 and (step % args.checkpoint_interval == 0 or step == args.train_steps):
            save_checkpoint("%s-%d.npz" % (checkpoint_path, step), trainer, corpus)
        if rank == 0 and step % args.eval_interval == 0:
            print("\nEvaluating at step {}".format(step))                     # predict_random_samples, train.py:114-139
            mel, wav = dataset.eval_sample()
            model = FloWaveNet(hparams, device=device, cond_mode=1).load_params(trainer.opt.master_views())
            g = torch.Generator().manual_seed(step)
            z = torch.randn(1, len(wav), 1, generator=g) * hparams.temp
            pred_dev = model.reverse(z, torch.from_numpy(mel[None])).reshape(-1)
            pred = pred_dev.cpu().numpy()
            write_wav(os.path.join(train_logdir, "predictions-%d.wav" % step), pred, hparams.sample_rate)
            write_wav(os.path.join(train_logdir, "targets-%d.wav" % step), wav, hparams.sample_rate)
            if bool(getattr(args, "eval_metrics", False)):                   # the same prediction against its target, on the device
                from .evaluate import eval_record
                from .metrics import SpectralDistance
                if eval_metric is None:
                    eval_metric = SpectralDistance(hparams, device=device)
                target = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32).reshape(-1)).to(pred_dev.device)
                eval_logdir = os.path.join(log_dir, "eval")
                os.makedirs(eval_logdir, exist_ok=True)
                log(eval_logdir, eval_record(step, eval_metric.dist(target, pred_dev)))
    return save_dir


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--base_dir", default="")
    parser.add_argument("--input", default="training_data/train.txt")
    parser.add_argument("--input_dir", default="training_data/", help="folder to contain inputs sentences/targets")
    parser.add_argument("--restore", type=lambda s: str(s).lower() not in ("false", "0", "no"), default=True,
                        help="Set this to False to do a fresh training")
    parser.add_argument("--summary_interval", type=int, default=500, help="Steps between running summary ops")
    parser.add_argument("--checkpoint_interval", type=int, default=2000, help="Steps between writing checkpoints")
    parser.add_argument("--eval_interval", type=int, default=5000, help="Steps between eval on test data")
    parser.add_argument("--train_steps", type=int, default=2000000, help="total number of model training steps")
    parser.add_argument("--log_dir", default="logs")
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--ragged", action="store_true",
                        help="also train on utterances shorter than max_time_steps, whole, with per-clip lengths; the ActNorm init "
                             "batch is full-length crops where the corpus has an utterance longer than max_time_steps, a ragged batch "
                             "where it has none")
    parser.add_argument("--ragged_init", action="store_true",
                        help="with --ragged: take the ActNorm init batch as a training batch is drawn (short utterances whole, with "
                             "their lengths) on any corpus")
    def positive(s):
        k = int(s)
        if k < 1:
            raise argparse.ArgumentTypeError("must be >= 1")
        return k

    parser.add_argument("--accum_steps", type=positive, default=1,
                        help="micro-batches per optimiser update: the gradients of K batches are summed and averaged into one "
                             "clip / Adam update (effective batch K x batch_size x ranks); steps and every interval count updates")
    parser.add_argument("--device_corpus", action="store_true",
                        help="upload the training utterances to the GPU once and draw every training batch there (a Philox stream "
                             "keyed by seed, rank and a draw counter on the device: not the host draws of a run without the flag); "
                             "checkpoints then carry the counter and a restored run continues the data stream; every rank holds the "
                             "whole corpus; combines with --ragged and --accum_steps")
    parser.add_argument("--eval_metrics", action="store_true",
                        help="at --eval_interval also measure the evaluation sample's prediction against its target on the device "
                             "(metrics.SpectralDistance: mel L1, log-spectral distance, spectral convergence) and append the "
                             "record to <log_dir>/eval/summary.jsonl; the two wavs are written as without the flag")
    args = parser.parse_args(argv)
    import torch
    import torch.distributed as dist
    from .hparams import hparams
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        dist.init_process_group("nccl")
    try:
        train(os.path.join(args.base_dir, args.log_dir), args, hparams, args.input)
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
