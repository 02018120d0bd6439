"""Mel front-end - the reference's ``preprocessing.py`` on MI355X.

Same names, file layout and value ranges as the reference (``preprocessing.py:13-106``):
``preprocess(in_dir, out_dir)`` writes ``audios/dataset-audio-%05d.npy`` (float32 samples, length a
multiple of ``hop_size``), ``mels/dataset-mel-%05d.npy`` (float32 ``[N, num_mels]`` in [0, 1]) and
``train.txt`` (``audio|mel|timesteps|speaker|text``); ``_process_utterance`` is the per-clip step.
The spectrogram (``librosa.feature.melspectrogram`` in the reference, ``:58-64``) runs in
``libfwn.so`` (``fwn_mel_spectrogram``); there is no CPU fallback.

Differences (deliberate): wavs are read with the stdlib ``wave`` module (``load_wav``: 8, 16, 24 and
32-bit PCM of any rate and channel count) and a wav whose rate is not ``hparams.sample_rate`` is
resampled on the device (``resample.Resampler`` - where the reference's ``librosa.load(...,
sr=hparams.sample_rate)`` resamples, ``:50``; librosa is not a dependency and its filter is not
reproduced: the definition is DESIGN.md "Sample-rate conversion"), so corpora of any rate and of
mixed rates go in; a corpus already at ``hparams.sample_rate`` gives the files it always gave.
``read_wav`` is the strict reader (16-bit at the model's rate, an error otherwise).  Non-PCM wav
encodings and compressed formats are out of scope; the TFRecord writer (``tfrecord.py``) is too, and
clips are processed on one device stream instead of a process pool.

Opt-in: ``MelFrontEnd`` does peak normalisation, the spectrogram (through an FFT in
LDS) and the reference's padding on the device for a ragged batch of clips in two launches;
``preprocess(..., batch=N)`` / ``--batch N`` reads the corpus N utterances at a time through it
(``audios/`` keep their bytes, ``mels/`` are the FFT's result, equal to the default path's within
float32 rounding); ``MelStream`` gives mel frames while audio is still arriving.  Without the flag
every launch and every bit is what it was.
"""
from __future__ import annotations

import os
import wave

import numpy as np

from . import _lib
from .rows import as_lengths, as_rows


def _mel_points(fmin, fmax, n):
    """n frequencies evenly spaced on the Slaney mel scale (linear to 1 kHz, log above)."""
    lin, knee, step = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0

    def to_mel(f):
        return f / lin if f < knee else knee / lin + np.log(f / knee) / step

    m = np.linspace(to_mel(float(fmin)), to_mel(float(fmax)), n)
    return np.where(m < knee / lin, m * lin, knee * np.exp(step * (m - knee / lin)))


def mel_filterbank(hparams):
    """Triangular, area-normalised (Slaney) filters: float32 [num_mels, n_fft/2 + 1]."""
    nb = hparams.n_fft // 2 + 1
    edges = _mel_points(hparams.fmin, hparams.fmax, hparams.num_mels + 2)
    freqs = np.arange(nb) * (hparams.sample_rate / float(hparams.n_fft))
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    tri = np.minimum((freqs[None, :] - lo) / (mid - lo), (hi - freqs[None, :]) / (hi - mid))
    return (np.maximum(tri, 0.0) * (2.0 / (hi - lo))).astype(np.float32)


def hann_window(n):
    """Periodic Hann window (scipy ``get_window('hann', n, fftbins=True)``), float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)


class MelSpectrogram:
    """``wav [B, T] -> mel [B, 1 + T // hop, num_mels]`` on the device (preprocessing.py:58-69)."""

    def __init__(self, hparams, device="cuda"):
        import torch
        self._hp = hparams
        self._lib = _lib.load()          # fails loudly when libfwn.so is missing
        self._device = torch.device(device)
        self._win = torch.from_numpy(hann_window(hparams.n_fft)).to(self._device)
        self._fb = torch.from_numpy(mel_filterbank(hparams)).to(self._device)

    def __call__(self, wav):
        import torch
        hp = self._hp
        w = torch.as_tensor(wav)
        squeeze = w.dim() == 1
        if squeeze:
            w = w[None]
        if w.dim() != 2:
            raise ValueError("wav must have shape [T] or [B, T], got %r" % (tuple(w.shape),))
        w = w.to(device=self._device, dtype=torch.float32).contiguous()
        b, t = int(w.shape[0]), int(w.shape[1])
        frames = 1 + t // hp.hop_size
        mel = torch.empty(b, frames, hp.num_mels, dtype=torch.float32, device=self._device)
        rc = self._lib.fwn_mel_spectrogram(w.data_ptr(), b, t, self._win.data_ptr(), self._fb.data_ptr(),
                                           hp.n_fft, hp.hop_size, hp.num_mels, float(hp.ref_level_db),
                                           float(hp.min_level_db), mel.data_ptr(),
                                           torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(rc, "fwn_mel_spectrogram")
        return mel[0] if squeeze else mel


def _process_utterance(wav, hparams, mel_fn=None):
    """One clip (preprocessing.py:49-89, minus the file I/O): float samples -> (audio, mel).

    audio: float32 [N * hop_size], zero padded / trimmed to the mel's frame count (:71-84);
    mel: float32 [N, num_mels] in [0, 1]."""
    wav = np.asarray(wav, dtype=np.float32)
    peak = float(np.abs(wav).max())
    if not peak > 0.0:
        raise ValueError("silent clip: the reference divides by max|wav| (preprocessing.py:52)")
    wav = wav / peak * hparams.rescaling_max
    mel_fn = mel_fn or MelSpectrogram(hparams)
    mel = mel_fn(wav).cpu().numpy()
    hop = hparams.hop_size
    pad = (len(wav) // hop + 1) * hop - len(wav)
    out = np.pad(wav, (pad // 2, pad // 2 + pad % 2))
    n = mel.shape[0]
    assert len(out) >= n * hop
    return out[:n * hop].astype(np.float32), mel.astype(np.float32)


def mel_bands(fb):
    """int32 ``[num_mels, 2]``: first and one-past-last non-zero bin of each row of ``fb`` (``[0, 0]`` for an empty row) - the
    ``bands`` table of ``fwn_mel_front``, which sums over those bins only."""
    bands = np.zeros((fb.shape[0], 2), dtype=np.int32)
    for m, row in enumerate(np.asarray(fb)):
        nz = np.flatnonzero(row)
        if len(nz):
            bands[m] = (nz[0], nz[-1] + 1)
    return bands


class MelFrontEnd:
    """The reference's per-clip step (``_process_utterance``: peak normalisation, spectrogram, padding) for a ragged batch on
    the device, DESIGN.md 6c: ``front(wav, lengths=None, normalize=True, audio=True)`` with ``wav`` float32 ``[T]`` or
    ``[B, T]`` and ``lengths`` (a list, or a device int64 tensor, ``[B]``) the clips' own lengths -> ``(audio [B, F hop] or
    None, mel [B, F, num_mels], peak [B])`` with ``F = 1 + T // hop``, all on the device: clip b's ``1 + lengths[b] // hop``
    frames and as many hops of padded audio, +0 behind them.  Two launches (``fwn_clip_peak``, ``fwn_mel_front``), no
    synchronisation; every clip gets the bits it gets alone.  ``normalize=False``: the samples as they are (``peak`` is still
    returned).  A silent or NaN clip, or one shorter than ``n_fft / 2 + 1`` samples, comes back as zeros: ``peak`` tells."""

    def __init__(self, hparams, device="cuda"):
        import torch
        self._hp = hparams
        self._lib = _lib.load()          # fails loudly when libfwn.so is missing
        self._device = torch.device(device)
        fb = mel_filterbank(hparams)
        self._fb = torch.from_numpy(fb).to(self._device)
        self._bands = torch.from_numpy(mel_bands(fb)).to(self._device)
        self.frames_per_workgroup = self._lib.fwn_mel_front_frames(hparams.n_fft, hparams.hop_size)
        if self.frames_per_workgroup < 0:
            _lib.check(self.frames_per_workgroup, "fwn_mel_front_frames")

    def __call__(self, wav, lengths=None, normalize=True, audio=True, bands=True):
        import torch
        hp = self._hp
        w = as_rows(wav, "wav", self._device)
        b, t = int(w.shape[0]), int(w.shape[1])
        lengths = as_lengths(lengths, b, self._device)
        frames = 1 + t // hp.hop_size
        peak = torch.empty(b, dtype=torch.float32, device=self._device)
        mel = torch.empty(b, frames, hp.num_mels, dtype=torch.float32, device=self._device)
        out = torch.empty(b, frames * hp.hop_size, dtype=torch.float32, device=self._device) if audio else None
        stream = torch.cuda.current_stream(self._device).cuda_stream
        len_ptr = None if lengths is None else lengths.data_ptr()
        _lib.check(self._lib.fwn_clip_peak(w.data_ptr(), b, t, len_ptr, t, peak.data_ptr(), stream), "fwn_clip_peak")
        rc = self._lib.fwn_mel_front(w.data_ptr(), b, t, len_ptr, t, peak.data_ptr() if normalize else None,
                                     float(hp.rescaling_max) if normalize else 1.0, self._fb.data_ptr(),
                                     self._bands.data_ptr() if bands else None, hp.n_fft, hp.hop_size, hp.num_mels,
                                     float(hp.ref_level_db), float(hp.min_level_db), mel.data_ptr(), frames * hp.num_mels,
                                     None if out is None else out.data_ptr(), frames * hp.hop_size, stream)
        _lib.check(rc, "fwn_mel_front")
        return out, mel, peak


class MelStream:
    """Mel frames of a clip that arrives in chunks: ``push(chunk)`` returns the frames that have become computable - those
    whose ``n_fft`` samples have arrived - as ``[k, num_mels]`` (or None), ``finish()`` the rest (their supports are reflected at
    the clip's end).  Concatenated they are ``MelFrontEnd(normalize=False)`` of the whole clip times ``gain``, bit for bit in any
    split: a frame's bits depend on the samples in its support only, so every call runs on a hop-aligned slice
    of the clip and keeps the frames that need no reflection inside the slice - except at the clip's true start and end.  At
    most ``n_fft + hop`` samples of history are kept.  No normalisation - a stream's peak is unknown until it ends: ``gain``
    is a plain multiplier applied on the host to every chunk, and mels for a model trained on normalised audio need the
    caller's gain.

    ``compute(samples)`` is the arithmetic: float32 ``[L]`` -> all ``1 + L // hop`` frames of that slice taken as a clip of its
    own; the default is a ``MelFrontEnd`` (chunks then come back as device tensors).  ``cat`` joins frame blocks.  Everything
    else here is integer planning on the host, so it runs without a device over a NumPy ``compute``."""

    def __init__(self, hparams, gain=1.0, compute=None, cat=None):
        self.n_fft, self.hop, self.gain = int(hparams.n_fft), int(hparams.hop_size), float(gain)
        self.h = self.n_fft // 2
        if compute is None:
            import torch
            front = MelFrontEnd(hparams)
            compute = lambda x: front(torch.from_numpy(x), normalize=False, audio=False)[1][0]      # noqa: E731
            cat = torch.cat
        self._compute, self._cat = compute, cat or np.concatenate
        self._hist = np.zeros(0, dtype=np.float32)      # clip samples [start, received)
        self.start = self.received = self.emitted = 0
        self._finished = False

    @property
    def retained(self):
        """Samples of history held right now."""
        return self.received - self.start

    def _slice_start(self, f):
        """The hop-aligned sample from which frame f on needs the clip: its support starts at f hop - n_fft / 2, and a frame
        reflected at the clip's end reaches one sample further back."""
        return max(0, (f * self.hop - self.h - 1) // self.hop * self.hop)

    def _emit(self, f_end):
        out = None
        if f_end > self.emitted:
            s0 = self._slice_start(self.emitted)
            g0 = self.emitted - s0 // self.hop
            out = self._compute(np.ascontiguousarray(self._hist[s0 - self.start:]))[g0:g0 + f_end - self.emitted]
            self.emitted = f_end
        keep = min(self.received, self._slice_start(self.emitted))
        if keep > self.start:
            self._hist = self._hist[keep - self.start:]
            self.start = keep
        return out

    def push(self, chunk):
        if self._finished:
            raise RuntimeError("push after finish")
        chunk = np.asarray(chunk, dtype=np.float32).reshape(-1)
        if self.gain != 1.0:
            chunk = chunk * np.float32(self.gain)
        if len(chunk):
            self._hist = np.concatenate([self._hist, chunk])
            self.received += len(chunk)
        # frame f is complete once sample f hop + n_fft / 2 - 1 has arrived (frame 0 reads sample n_fft / 2: its reflection)
        f_end = (self.received - self.h) // self.hop + 1 if self.received >= self.h + 1 else 0
        return self._emit(max(self.emitted, f_end))

    def finish(self):
        if self._finished:
            raise RuntimeError("finish called twice")
        self._finished = True
        if self.received < self.h + 1:
            raise ValueError("a clip of %d samples cannot be reflect-padded: n_fft / 2 + 1 = %d are needed" % (self.received, self.h + 1))
        out = self._emit(1 + self.received // self.hop)
        self._hist = None
        return out


def read_wav(path, sample_rate):
    """16-bit PCM wav at ``sample_rate`` -> float32 mono in [-1, 1)."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: only 16-bit PCM is supported" % path)
        if w.getframerate() != sample_rate:
            raise ValueError("%s: sample rate %d != hparams.sample_rate %d (resample first)"
                             % (path, w.getframerate(), sample_rate))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / 32768.0
        if w.getnchannels() > 1:
            pcm = pcm.reshape(-1, w.getnchannels()).mean(axis=1)
    return pcm


def _pcm_to_float(raw, width, path="wav"):
    """The bytes of little-endian PCM frames -> float32 in [-1, 1): 8-bit is unsigned ((v - 128) / 128), 16, 24 and 32-bit are
    signed (v / 2^(bits - 1)).  8, 16 and 24-bit values are exact in float32; 32-bit ones are divided in float64 and rounded once
    (the largest few then round to 1.0)."""
    if width == 1:
        return (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    if width == 2:
        return np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    if width == 4:
        return (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    raise ValueError("%s: %d-byte samples are not supported (8, 16, 24 and 32-bit PCM are)" % (path, width))


def _read_pcm(path):
    """PCM wav -> (float32 mono at the file's own rate, that rate): ``load_wav`` before it resamples."""
    with wave.open(path, "rb") as w:
        rate, channels = w.getframerate(), w.getnchannels()
        pcm = _pcm_to_float(w.readframes(w.getnframes()), w.getsampwidth(), path)
    if channels > 1:
        pcm = pcm.reshape(-1, channels).mean(axis=1)
    return pcm, rate


def load_wav(path, sample_rate, resamplers=None):
    """PCM wav of any rate -> float32 mono at ``sample_rate`` (the reference's ``librosa.load(path, sr=sample_rate)``).

    8, 16, 24 and 32-bit PCM through the stdlib ``wave`` module; the channel mean as ``read_wav`` takes it; a file whose rate
    differs is resampled on the device (``resample.Resampler``).  ``resamplers``: a dict the caller keeps, source rate ->
    ``Resampler``, so that a corpus designs and uploads one table per source rate.  A 16-bit file at ``sample_rate`` gives
    ``read_wav``'s array bit for bit, with no device call."""
    pcm, rate = _read_pcm(path)
    if rate == int(sample_rate):
        return pcm
    from .resample import Resampler
    if resamplers is None:
        resamplers = {}
    if rate not in resamplers:
        resamplers[rate] = Resampler(rate, sample_rate)
    if len(pcm) == 0:
        return pcm
    import torch
    return resamplers[rate](torch.from_numpy(np.ascontiguousarray(pcm))).cpu().numpy()


def _corpus_lines(in_dir):
    """``(wav path, text)`` of every utterance in index order: the books sorted, each ``metadata.csv`` top to bottom."""
    books = sorted(os.path.join(in_dir, f) for f in os.listdir(in_dir) if os.path.isdir(os.path.join(in_dir, f)))
    for book in books:
        with open(os.path.join(book, "metadata.csv"), encoding="utf-8") as f:
            lines = f.read().strip().split("\n")
        for line in lines:
            parts = line.strip().split("|")
            yield os.path.join(book, "wavs", "%s.wav" % parts[0]), parts[2] if len(parts) > 2 else ""


def ragged_rows(clips, device):
    """Host float32 clips of different lengths -> (device float32 ``[B, max length]`` zero padded, their lengths): one upload."""
    import torch
    lengths = [len(c) for c in clips]
    x = np.zeros((len(clips), max(max(lengths), 1)), dtype=np.float32)
    for row, c in enumerate(clips):
        x[row, :len(c)] = c
    return torch.from_numpy(x).to(device), lengths


def load_wavs(paths, sample_rate, resamplers, device="cuda"):
    """``load_wav`` for a batch: -> (device float32 ``[B, T]``, lengths).  The files at ``sample_rate`` go up as they are; the
    others are resampled per source rate in one ragged ``Resampler`` call each and stay on the device."""
    from .resample import Resampler
    read = [_read_pcm(p) for p in paths]
    out_len, by_rate = [], {}
    for row, (pcm, rate) in enumerate(read):
        if rate == int(sample_rate):
            out_len.append(len(pcm))
        else:
            if rate not in resamplers:
                resamplers[rate] = Resampler(rate, sample_rate, device=device)
            out_len.append(resamplers[rate].out_length(len(pcm)))
            by_rate.setdefault(rate, []).append(row)
    import torch
    host = np.zeros((len(read), max(max(out_len), 1)), dtype=np.float32)
    for row, (pcm, rate) in enumerate(read):
        if rate == int(sample_rate):
            host[row, :len(pcm)] = pcm
    x = torch.from_numpy(host).to(device)
    for rate, rows in by_rate.items():
        src, src_len = ragged_rows([read[row][0] for row in rows], device)
        if max(src_len) == 0:
            continue
        y = resamplers[rate](src, lengths=src_len)
        for j, row in enumerate(rows):
            x[row, :out_len[row]] = y[j, :out_len[row]]
    return x, out_len


def _build_batched(in_dir, out_dir, hparams, batch):
    """``build_from_path`` through ``MelFrontEnd``, ``batch`` utterances per call: one front-end call and one download per batch."""
    import torch
    if int(batch) < 1:
        raise ValueError("batch must be a positive number of utterances, got %r" % (batch,))
    front = MelFrontEnd(hparams)
    resamplers = {}
    hop = hparams.hop_size
    lines = list(_corpus_lines(in_dir))
    metadata = []
    for i in range(0, len(lines), int(batch)):
        group = lines[i:i + int(batch)]
        x, lengths = load_wavs([path for path, _ in group], hparams.sample_rate, resamplers)
        audio, mel, peak = front(x, lengths=lengths)
        flat = torch.cat([audio.reshape(-1), mel.reshape(-1), peak]).cpu().numpy()       # the one download
        b, na, nm = len(group), audio[0].numel(), mel[0].numel()
        audio, mel, peak = flat[:b * na].reshape(b, na), flat[b * na:b * (na + nm)].reshape(b, -1, hparams.num_mels), flat[b * (na + nm):]
        for (path, _), pk in zip(group, peak):
            if not pk > 0.0:
                raise ValueError("%s: silent clip: the reference divides by max|wav| (preprocessing.py:52)" % path)
        for row, (path, text) in enumerate(group):
            index = i + row + 1
            frames = 1 + lengths[row] // hop
            audio_filename = "dataset-audio-%05d.npy" % index
            mel_filename = "dataset-mel-%05d.npy" % index
            np.save(os.path.join(out_dir, "audios", audio_filename), audio[row, :frames * hop], allow_pickle=False)
            np.save(os.path.join(out_dir, "mels", mel_filename), mel[row, :frames], allow_pickle=False)
            metadata.append((audio_filename, mel_filename, frames * hop, 0, text))
    return metadata


def build_from_path(in_dir, out_dir, hparams, num_workers=1, batch=None):
    """``in_dir/<book>/metadata.csv`` + ``wavs/<id>.wav`` (single speaker, preprocessing.py:30-45).  ``batch``: opt-in, the
    utterances ``batch`` at a time through ``MelFrontEnd``; None is the per-clip path as it always was."""
    del num_workers     # one device stream does the work of the reference's process pool
    if batch is not None:
        return _build_batched(in_dir, out_dir, hparams, batch)
    mel_fn = MelSpectrogram(hparams)
    resamplers = {}                                  # one Resampler (one phase table on the device) per source rate
    books = sorted(os.path.join(in_dir, f) for f in os.listdir(in_dir) if os.path.isdir(os.path.join(in_dir, f)))
    metadata, index = [], 1
    for book in books:
        with open(os.path.join(book, "metadata.csv"), encoding="utf-8") as f:
            lines = f.read().strip().split("\n")
        for line in lines:
            parts = line.strip().split("|")
            text = parts[2] if len(parts) > 2 else ""
            wav = load_wav(os.path.join(book, "wavs", "%s.wav" % parts[0]), hparams.sample_rate, resamplers)
            audio, mel = _process_utterance(wav, hparams, mel_fn)
            audio_filename = "dataset-audio-%05d.npy" % index
            mel_filename = "dataset-mel-%05d.npy" % index
            np.save(os.path.join(out_dir, "audios", audio_filename), audio, allow_pickle=False)
            np.save(os.path.join(out_dir, "mels", mel_filename), mel, allow_pickle=False)
            metadata.append((audio_filename, mel_filename, len(audio), 0, text))
            index += 1
    return metadata


def write_metadata(metadata, out_dir, hparams):
    with open(os.path.join(out_dir, "train.txt"), "w", encoding="utf-8") as f:
        for m in metadata:
            f.write("|".join(str(x) for x in m) + "\n")
    frames = sum(m[2] for m in metadata)
    print("Wrote %d utterances, %d time steps (%.2f hours)"
          % (len(metadata), frames, frames / hparams.sample_rate / 3600))
    print("Max input length:  %d" % max(len(m[4]) for m in metadata))
    print("Max output length: %d" % max(m[2] for m in metadata))


def preprocess(in_dir, out_dir, hparams=None, num_workers=1, batch=None):
    if hparams is None:
        from .hparams import hparams as hparams_default
        hparams = hparams_default
    for sub in ("", "audios", "mels"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    metadata = build_from_path(in_dir, out_dir, hparams, num_workers, batch)
    write_metadata(metadata, out_dir, hparams)
    return metadata


def _batch_arg(text):
    import argparse
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError("a positive number of utterances, got %r" % (text,))
    return n


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Preprocessing",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--in_dir", "-i", type=str, default="./", help="In Directory")
    parser.add_argument("--out_dir", "-o", type=str, default="./", help="Out Directory")
    # absent from the namespace unless given: without the flag the arguments are what they were
    parser.add_argument("--batch", type=_batch_arg, default=argparse.SUPPRESS, metavar="N",
                        help="read N utterances at a time through the device front-end (MelFrontEnd: peak, FFT spectrogram and "
                             "padding in two launches per batch); default: one utterance per launch, as ever")
    return parser.parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    preprocess(args.in_dir, args.out_dir, batch=getattr(args, "batch", None))
