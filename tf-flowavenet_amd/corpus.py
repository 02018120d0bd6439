"""Device-resident training corpus (``train.py --device_corpus``): the utterances are uploaded once and every batch is drawn
and gathered by ``fwn_corpus_draw`` on the training stream - no per-step host work, nothing over PCIe, and a draw counter on
the device that a checkpoint can hold.

``CorpusLayout`` is the host half: the eligible training utterances of a ``train.Dataset`` (its own rule, its own split) laid
out as fwn.h describes - audio back to back, mel rows back to back, one int64 table of frame offsets, utterance ``u`` holding
``min(mel frames, audio samples // hop)`` frames.  ``DeviceCorpus`` uploads that and draws.  The stream is this project's own
(Philox4x32-10 keyed by seed, rank and the counter; include/fwn.h has the definition, tests/corpus_ref.py restates it): it is
NOT ``Dataset``'s ``RandomState`` stream, so a run with the flag sees other batches than a run without it.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib

COUNTER_KEY = "__data/draw_counter"      # the optional checkpoint entry: uint64, the number of draws made so far
_CHUNK_BYTES = 64 << 20                  # host staging per upload


class CorpusLayout:
    """The training split of ``dataset`` (a ``train.Dataset``) as a flat corpus: ``frame_off`` int64 [n_utt + 1], ``hop``,
    ``num_mels``, ``frames`` (F = max_time_steps // hop), ``unit_frames``, ``ragged`` - all host-side, nothing read but the
    ``.npy`` headers until ``utterance`` / ``arrays`` are called."""

    def __init__(self, dataset):
        hp = dataset._hp
        self.dataset, self.hop, self.num_mels = dataset, int(hp.hop_size), int(hp.num_mels)
        self.frames, self.unit_frames, self.ragged = int(dataset._frames), int(dataset._unit_frames()), bool(dataset._ragged)
        self.meta = list(dataset.train_meta)
        counts = []
        for m in self.meta:
            audio, mel = self._open(m)
            if mel.ndim != 2 or mel.shape[1] != self.num_mels:
                raise ValueError("%s: mel of shape %s, expected [frames, %d]" % (m[1], tuple(mel.shape), self.num_mels))
            n = min(int(mel.shape[0]), len(audio) // self.hop)
            if not self.ragged and n <= self.frames:
                # the draw would take it whole and report a shorter length, which a step without lengths cannot honour
                raise ValueError("%s holds %d common frames of mel and audio, not more than max_time_steps // hop_size = %d: "
                                 "use --ragged or drop it" % (m[0], n, self.frames))
            counts.append(n)
            del audio, mel
        self.frame_off = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)
        self.n_utt, self.total_frames = len(counts), int(self.frame_off[-1])
        self.audio_bytes = 4 * self.total_frames * self.hop
        self.mel_bytes = 4 * self.total_frames * self.num_mels
        self.nbytes = self.audio_bytes + self.mel_bytes + 8 * (self.n_utt + 1)

    def _open(self, m):
        """(audio, mel) of one metadata row without going through ``Dataset._load``'s LRU of open maps: TFRecord samples are
        resident in the dataset, ``.npy`` files are memory-mapped here and dropped by the caller."""
        ds = self.dataset
        hit = ds._cache.get(m[0])
        if hit is not None:
            return hit
        return (np.load(os.path.join(ds._basedir, "audios", m[0]), mmap_mode="r"),
                np.load(os.path.join(ds._basedir, "mels", m[1]), mmap_mode="r"))

    def utterance(self, u):
        """-> (audio float32 [n * hop], mel float32 [n, num_mels]) of utterance u, cut to its n common frames (copies)."""
        n = int(self.frame_off[u + 1] - self.frame_off[u])
        audio, mel = self._open(self.meta[u])
        return (np.ascontiguousarray(audio[:n * self.hop], dtype=np.float32).reshape(-1),
                np.ascontiguousarray(mel[:n], dtype=np.float32))

    def chunks(self, limit=_CHUNK_BYTES):
        """Yields ``(first_frame, audio, mel)`` for runs of whole utterances of about ``limit`` bytes: the upload's staging."""
        per_frame = 4 * (self.hop + self.num_mels)
        u = 0
        while u < self.n_utt:
            v = u + 1
            while v < self.n_utt and (self.frame_off[v + 1] - self.frame_off[u]) * per_frame <= limit:
                v += 1
            parts = [self.utterance(k) for k in range(u, v)]
            yield (int(self.frame_off[u]), np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts], axis=0))
            u = v

    def arrays(self):
        """-> (audio float32 [total_frames * hop], mel float32 [total_frames, num_mels]) on the host (tests; small corpora)."""
        audio = np.empty(self.total_frames * self.hop, dtype=np.float32)
        mel = np.empty((self.total_frames, self.num_mels), dtype=np.float32)
        for f0, a, m in self.chunks():
            audio[f0 * self.hop:f0 * self.hop + len(a)] = a
            mel[f0:f0 + len(m)] = m
        return audio, mel


def open_dataset(path, hparams, seed=None, rank=0, ragged=False):
    """The ``train.Dataset`` of ``train.txt`` or ``train.tfrecord`` at ``path``, as ``train.train`` opens it."""
    from .train import Dataset
    if path.endswith(".tfrecord"):
        return Dataset.from_tfrecords(path, os.path.join(os.path.dirname(path), "test.tfrecord"), hparams, seed=seed, rank=rank,
                                      ragged=ragged)
    return Dataset(path, hparams, seed=seed, rank=rank, ragged=ragged)


class DeviceCorpus:
    """The training split on the device and the draw from it.

    dataset_or_meta: a ``train.Dataset`` (its ``train_meta`` IS the eligible set: strictly more than ``max_time_steps // hop``
    frames, or with ``ragged`` at least one unit) or the path of a ``train.txt`` / ``train.tfrecord``, opened as ``train.py``
    opens it.  seed: None takes ``hparams.shuffle_random_seed``; rank is the draw's ``stream_id`` - every rank of a
    data-parallel run holds the whole corpus and draws its own slots.  ragged: None takes the dataset's mode.
    Raises ``MemoryError`` with the byte count, before anything is uploaded, when the arrays do not fit the device's free
    memory (``max_bytes`` overrides what counts as free)."""

    def __init__(self, dataset_or_meta, hparams, seed=None, rank=0, ragged=None, device="cuda", max_bytes=None):
        import torch
        if isinstance(dataset_or_meta, (str, os.PathLike)):
            dataset_or_meta = open_dataset(os.fspath(dataset_or_meta), hparams, seed=seed, rank=rank, ragged=bool(ragged))
        elif ragged is not None and bool(ragged) != bool(dataset_or_meta._ragged):
            raise ValueError("DeviceCorpus: ragged=%r, but the dataset was opened with ragged=%r" % (ragged, dataset_or_meta._ragged))
        self.layout = lay = CorpusLayout(dataset_or_meta)
        self.hp, self.ragged = hparams, lay.ragged
        self.seed = int(hparams.shuffle_random_seed if seed is None else seed) % (1 << 64)
        self.stream_id = int(rank) & 0xFFFFFFFF
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        free = int(torch.cuda.mem_get_info(self.device)[0]) if max_bytes is None else int(max_bytes)
        if lay.nbytes > free:
            raise MemoryError("DeviceCorpus: the corpus takes %d bytes (%d of audio, %d of mels, %d utterances) and %d are free on %s"
                              % (lay.nbytes, lay.audio_bytes, lay.mel_bytes, lay.n_utt, free, self.device))
        self.audio = torch.empty(lay.total_frames * lay.hop, dtype=torch.float32, device=self.device)
        self.mel = torch.empty(lay.total_frames, lay.num_mels, dtype=torch.float32, device=self.device)
        for f0, a, m in lay.chunks():
            self.audio[f0 * lay.hop:f0 * lay.hop + len(a)].copy_(torch.from_numpy(a))
            self.mel[f0:f0 + len(m)].copy_(torch.from_numpy(m))
        self.frame_off = torch.from_numpy(lay.frame_off).to(self.device)
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)       # the uint64's bits
        self._out = {}
        self.picks = None

    # ------------------------------------------------------------------ the draw
    def draw(self, batch_size):
        """-> ``(x [B, F * hop], c [B, F, num_mels], lengths)`` on the device, drawn on the current stream; ``lengths`` is a
        ``training.DeviceLengths`` when ragged, else None (every clip is then F * hop samples by construction).  The same
        tensors are written by every call at a batch size - consume a batch (in stream order) before drawing the next -
        and ``picks`` is the int32 [B, 2] table ``(utterance, start frame)`` of the last draw."""
        import torch
        from .training import DeviceLengths
        b, lay = int(batch_size), self.layout
        out = self._out.get(b)
        if out is None:
            x = torch.empty(b, lay.frames * lay.hop, dtype=torch.float32, device=self.device)
            c = torch.empty(b, lay.frames, lay.num_mels, dtype=torch.float32, device=self.device)
            ln = torch.empty(b, dtype=torch.int32, device=self.device)
            picks = torch.empty(b, 2, dtype=torch.int32, device=self.device)
            out = self._out[b] = (x, c, ln, picks, DeviceLengths(ln) if self.ragged else None)
        x, c, ln, picks, lengths = out
        rc = self.lib.fwn_corpus_draw(self.audio.data_ptr(), self.mel.data_ptr(), self.frame_off.data_ptr(), lay.n_utt, lay.hop,
                                      lay.num_mels, lay.unit_frames, b, lay.frames, self.seed, self.stream_id,
                                      self._counter.data_ptr(), x.data_ptr(), c.data_ptr(), ln.data_ptr(), picks.data_ptr(),
                                      torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "fwn_corpus_draw")
        self.picks = picks
        return x, c, lengths

    # ------------------------------------------------------------------ the counter
    @property
    def counter(self):
        """The number of draws made so far (uint64).  Reading it synchronises: for checkpoints only."""
        return int(self._counter.item()) % (1 << 64)

    def set_counter(self, n):
        """The next draw is draw ``n`` (taken mod 2^64), in stream order."""
        n = int(n) % (1 << 64)
        self._counter.fill_(n - (1 << 64) if n >= (1 << 63) else n)
