"""Spectral denoiser on the device (``fwn_denoise`` / ``fwn_stft_mean_mag``, csrc/denoise.hip; DESIGN.md 6b has the definition,
tests/denoise_ref.py restates it in fp64).

A flow vocoder run at ``temp < 1`` adds a stationary, input-independent residue to every clip - its response to "nothing".  The
remedy is bias-spectrum subtraction: synthesize once from a zero latent and an all-zero mel, take the mean magnitude spectrum of
that clip's interior STFT frames as the model's bias ``b[k]``, and soft-threshold the magnitude of every STFT bin of every output
by ``strength * b[k]``, the phase kept; the inverse STFT is a least-squares overlap-add.  ``Denoiser`` holds ``b`` on the device
and is the one call; there is no host maths and no torch maths on the path.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .rows import as_lengths, as_rows, check_shape      # noqa: F401  (check_shape is part of this module's interface)


def check_strength(strength):
    s = float(strength)
    if not 0.0 <= s < float("inf"):                  # a NaN fails both
        raise ValueError("strength must be a finite number >= 0, got %r" % (strength,))
    return s


def strength_arg(text):
    """argparse type of ``--denoise``: a finite float >= 0 (anything else is a parser error)."""
    import argparse
    try:
        return check_strength(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


class Denoiser:
    """``Denoiser(model)`` computes the bias of ``model`` (a ``FloWaveNet`` with its parameters loaded): ``model.reverse`` of a
    zero latent and an all-zero mel of ``bias_frames`` frames (rounded up to the model's alignment), then ``fwn_stft_mean_mag``
    over that clip's interior frames.  The bias is a constant of the model's parameters: build a new ``Denoiser`` after
    ``load_params``.  ``Denoiser(bias=b, n_fft=, hop=)`` takes a caller's ``b`` ([n_fft / 2 + 1], finite, >= 0) instead.
    ``n_fft`` / ``hop`` default to the model's ``hparams.n_fft`` / hop size.

    ``denoiser(x, lengths=None, pcm=False, strength=None)``: ``x`` float32 ``[T]`` or ``[B, T]`` on the device; ``lengths`` (a
    list, or a device int64 tensor ``[B]``; clamped to ``[0, T]`` on the device) the clips' own lengths - nothing past a clip's
    length is read, and the result is 0 from there on; -> float32, or int16 PCM (``fwn_pcm16``'s arithmetic on the float result)
    with ``pcm=True``, of x's shape, on the current stream.  A clip shorter than ``n_fft / 2 + 1`` samples comes back unchanged."""

    def __init__(self, model=None, strength=0.01, n_fft=None, hop=None, bias=None, bias_frames=64, device=None):
        import torch
        if (model is None) == (bias is None):
            raise ValueError("give either a model (its bias is computed) or bias= (yours), not %s" % ("both" if bias is not None else "neither"))
        self.strength = check_strength(strength)
        if model is not None:
            hp = model._hparams
            n_fft = hp.n_fft if n_fft is None else n_fft
            hop = model.hop if hop is None else hop
            device = model._device if device is None else device
        elif n_fft is None or hop is None:
            raise ValueError("bias= needs n_fft= and hop= too")
        self.n_fft, self.hop = check_shape(n_fft, hop)
        self.nb = self.n_fft // 2 + 1
        self._lib = _lib.load()          # fails loudly when libfwn.so is missing
        self._device = torch.device("cuda" if device is None else device)
        if bias is not None:
            b = bias.detach().cpu().numpy() if hasattr(bias, "detach") else np.asarray(bias)
            if b.shape != (self.nb,):
                raise ValueError("bias must have shape [%d] (n_fft / 2 + 1), got %r" % (self.nb, tuple(b.shape)))
            b = b.astype(np.float32)
            if not (np.isfinite(b).all() and (b >= 0.0).all()):
                raise ValueError("bias must be finite and non-negative")
            self.bias = torch.from_numpy(b).to(self._device)
        else:
            self.bias = self._model_bias(model, int(bias_frames))

    def _model_bias(self, model, bias_frames):
        import torch
        if bias_frames < 1:
            raise ValueError("bias_frames must be positive, got %r" % (bias_frames,))
        hp = model._hparams
        unit = 1 << hp.n_block
        align = max(1, unit // int(np.gcd(unit, model.hop)))
        frames = bias_frames + (-bias_frames) % align
        z = torch.zeros(1, frames * model.hop, 1, dtype=torch.float32, device=self._device)
        c = torch.zeros(1, frames, hp.num_mels, dtype=torch.float32, device=self._device)
        self.bias_audio = model.reverse(z, c)[:, :, 0].contiguous()          # kept: what the bias was measured on
        return self.mean_mag(self.bias_audio)

    def mean_mag(self, x):
        """float32 ``[B, T]`` (or ``[T]``) on the device -> ``[nb]``: the mean magnitude over the rows' interior frames."""
        import torch
        x = as_rows(x, "x", self._device, strict=True)
        out = torch.empty(self.nb, dtype=torch.float32, device=self._device)
        rc = self._lib.fwn_stft_mean_mag(x.data_ptr(), int(x.shape[0]), int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]),
                                         int(x.shape[1]), self.n_fft, self.hop, out.data_ptr(),
                                         torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(rc, "fwn_stft_mean_mag")
        return out

    def __call__(self, x, lengths=None, pcm=False, strength=None):
        import torch
        squeeze = torch.as_tensor(x).dim() == 1
        x = as_rows(x, "x", self._device, strict=True)
        b, t = int(x.shape[0]), int(x.shape[1])
        s = self.strength if strength is None else check_strength(strength)
        lengths = as_lengths(lengths, b, self._device)
        out = torch.empty(b, t, dtype=torch.int16 if pcm else torch.float32, device=self._device)
        rc = self._lib.fwn_denoise(x.data_ptr(), b, t, None if lengths is None else lengths.data_ptr(), t, self.bias.data_ptr(), s,
                                   self.n_fft, self.hop, None if pcm else out.data_ptr(), t, out.data_ptr() if pcm else None, t,
                                   None, 0, torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(rc, "fwn_denoise")
        return out[0] if squeeze else out
