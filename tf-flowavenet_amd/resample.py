"""Sample-rate conversion on the device: one band-limited rational resampler (``fwn_resample``, csrc/resample.hip).

The reference resamples in its loader (``librosa.load(wav_path, sr=hparams.sample_rate)``, preprocessing.py:50); librosa is not
a dependency here and its filter is not reproduced.  The definition is this package's own (DESIGN.md "Sample-rate
conversion", restated in fp64 by tests/resample_ref.py): for ``in_rate -> out_rate`` with ``up / down`` the ratio in lowest
terms, a zero-phase Kaiser-windowed sinc of ``zeros`` zero crossings per side on the up-sampled grid, cut at ``rolloff`` of the
narrower Nyquist; a clip of N samples gives ``ceil(N up / down)`` outputs, the clip taken as 0 outside itself.

``Resampler`` is the device call; ``ResampleStream`` cuts a clip that arrives in chunks into calls whose outputs are, bit for
bit, those of one call over the whole clip (an output's bits depend on the samples in its support, on the clip's length and on
its own index only).  Its planning is host code over a compute step given to it, so it runs without a device too.
"""
from __future__ import annotations

import ctypes as C
from math import gcd

import numpy as np

from . import _lib
from .rows import as_lengths, as_rows

ZEROS, BETA, ROLLOFF = 32, 10.0, 0.90


def ratio(in_rate, out_rate):
    """``(up, down)``: out_rate / in_rate in lowest terms."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate < 1 or out_rate < 1:
        raise ValueError("sample rates must be positive, got %r -> %r" % (in_rate, out_rate))
    g = gcd(in_rate, out_rate)
    return out_rate // g, in_rate // g


def out_length(n, up, down):
    """ceil(n up / down): the outputs of a clip of n samples."""
    return -((-int(n) * int(up)) // int(down))


def design_table(up, down, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """The phase table float32 ``[up, K]`` from ``fwn_resample_design`` (host code: works without a GPU)."""
    lib = _lib.load()
    k = lib.fwn_resample_taps(int(up), int(down), int(zeros))
    if k < 0:
        _lib.check(k, "fwn_resample_taps")
    table = np.zeros((int(up), k), dtype=np.float32)
    _lib.check(lib.fwn_resample_design(int(up), int(down), int(zeros), float(beta), float(rolloff),
                                       table.ctypes.data_as(C.c_void_p)), "fwn_resample_design")
    return table


class ResampleStream:
    """A clip that arrives in chunks: ``push(chunk)`` returns the outputs that have become computable - those whose whole
    support has arrived -, ``finish()`` the rest (their supports end at the clip's end).  Concatenated, they are the one-call
    result exactly.  Only the samples a later output can still read are kept: fewer than ``2 Hh / up + down / up + 2``.

    ``compute(hist, in_start, n_total, m0, n_out)`` is the arithmetic: ``hist`` holds clip samples ``[in_start, in_start +
    len(hist))`` of a clip declared ``n_total`` long, and it returns outputs ``[m0, m0 + n_out)``.  ``cat(list)`` joins chunks
    (``np.concatenate`` / ``torch.cat``).  Everything else here is integer planning on the host."""

    def __init__(self, up, down, zeros, compute, cat=np.concatenate):
        self.up, self.down = int(up), int(down)
        self.hh = int(zeros) * max(self.up, self.down)
        self._compute, self._cat = compute, cat
        self._hist = None                  # clip samples [start, received)
        self.start = self.received = self.emitted = 0
        self._finished = False

    @property
    def retained(self):
        """Samples of history held right now."""
        return self.received - self.start

    def _emit(self, m_end, n_total):
        out = None
        if m_end > self.emitted:
            out = self._compute(self._hist, self.start, n_total, self.emitted, m_end - self.emitted)
            self.emitted = m_end
        # the lowest sample any later output reads: ceil((emitted down - Hh) / up)
        keep = min(self.received, max(self.start, -((self.hh - self.emitted * self.down) // self.up)))
        if keep > self.start:
            self._hist = self._hist[keep - self.start:]
            self.start = keep
        return out

    def push(self, chunk):
        if self._finished:
            raise RuntimeError("push after finish")
        if len(chunk):
            self._hist = chunk if self._hist is None or len(self._hist) == 0 else self._cat([self._hist, chunk])
            self.received += len(chunk)
        # output m is complete once sample floor((m down + Hh) / up) has arrived: m down + Hh < received up
        m_end = max(self.emitted, (self.received * self.up - self.hh - 1) // self.down + 1)
        return self._emit(m_end, self.received)

    def finish(self):
        if self._finished:
            raise RuntimeError("finish called twice")
        self._finished = True
        out = self._emit(out_length(self.received, self.up, self.down), self.received)
        self._hist = None
        return out


class Resampler:
    """``in_rate -> out_rate`` on the device.  The phase table is designed by ``fwn_resample_design`` and uploaded once.

    ``resampler(x, lengths=None)``: ``x`` float32 or int16 (PCM, read as ``v / 32768``) of shape ``[T]`` or ``[B, T]`` ->
    float32 ``[n_out(T)]`` or ``[B, n_out(T)]``; ``lengths`` (a list, or a device int64 tensor, ``[B]``) are the clips' own
    lengths: row b is resampled as a clip of ``lengths[b]`` samples - nothing past it is read - and is 0 from
    ``out_length(lengths[b])`` on.  Equal rates: the input's values as float32, no launch."""

    def __init__(self, in_rate, out_rate, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF, device="cuda"):
        import torch
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.up, self.down = ratio(in_rate, out_rate)
        self.zeros = int(zeros)
        self._lib = _lib.load()          # fails loudly when libfwn.so is missing
        self._device = torch.device(device)
        self.identity = self.up == 1 and self.down == 1
        self.taps, self._table = 1, None
        if not self.identity:
            table = design_table(self.up, self.down, zeros, beta, rolloff)
            self.taps = int(table.shape[1])
            self._table = torch.from_numpy(table).to(self._device)

    def out_length(self, n):
        return out_length(n, self.up, self.down)

    def run(self, x, in_start, n_total, m0, n_out, lengths=None):
        """One ``fwn_resample`` launch.  ``x`` ``[B, n_in]`` (float32 / int16, on the device, rows contiguous) holds clip samples
        ``[in_start, in_start + n_in)``; the clips are ``n_total`` long (``lengths``: device int64 ``[B]``, clamped to it); ->
        float32 ``[B, n_out]``: outputs ``[m0, m0 + n_out)``."""
        import torch
        if x.dtype not in (torch.float32, torch.int16):
            raise TypeError("x must be float32 or int16, got %s" % x.dtype)
        b, n_in = int(x.shape[0]), int(x.shape[1])
        y = torch.empty(b, int(n_out), dtype=torch.float32, device=self._device)
        if n_out == 0 or b == 0:
            return y
        rc = self._lib.fwn_resample(x.data_ptr(), int(x.dtype == torch.int16), b, int(x.stride(0)) if b > 1 else n_in, int(in_start),
                                    n_in, None if lengths is None else lengths.data_ptr(), int(n_total), self._table.data_ptr(),
                                    self.up, self.down, self.zeros, y.data_ptr(), int(n_out), int(m0), int(n_out),
                                    torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(rc, "fwn_resample")
        return y

    def __call__(self, x, lengths=None):
        import torch
        squeeze = torch.as_tensor(x).dim() == 1
        x = as_rows(x, "x", self._device, pcm16=True)
        b, t = int(x.shape[0]), int(x.shape[1])
        lengths = as_lengths(lengths, b, self._device)
        if self.identity:
            y = x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x
            if lengths is not None:
                y = torch.where(torch.arange(t, device=self._device)[None] < lengths[:, None], y, torch.zeros_like(y))
        else:
            y = self.run(x, 0, t, 0, self.out_length(t), lengths)
        return y[0] if squeeze else y

    def stream(self):
        """A ``ResampleStream`` over this resampler: chunks are 1-D device tensors (float32 or int16, one dtype per stream)."""
        import torch

        def compute(hist, in_start, n_total, m0, n_out):
            return self.run(hist[None], in_start, n_total, m0, n_out)[0]

        if self.identity:
            raise ValueError("equal rates: there is nothing to stream")
        return ResampleStream(self.up, self.down, self.zeros, compute, cat=torch.cat)
