"""What the audio units' device calls share on the Python side (``Denoiser``, ``SpectralDistance``, ``MelFrontEnd``,
``Resampler``): the STFT shape check, and a batch of clips as contiguous device rows with its lengths."""
from __future__ import annotations


def check_shape(n_fft, hop):
    n_fft, hop = int(n_fft), int(hop)
    if n_fft < 32 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError("n_fft must be a power of two in 32..4096, got %r" % (n_fft,))
    if not 1 <= hop <= n_fft // 2:
        raise ValueError("hop must be in 1..n_fft/2 = %d, got %r" % (n_fft // 2, hop))
    return n_fft, hop


def as_rows(x, name, device, strict=False, pcm16=False):
    """``[T]`` or ``[B, T]`` -> contiguous float32 ``[B, T]`` rows on ``device``; with ``pcm16`` an int16 input stays int16.  Any
    other dtype is converted - or, with ``strict``, refused (``TypeError``), and so are empty rows (``ValueError``)."""
    import torch
    x = torch.as_tensor(x)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or (strict and (x.shape[0] < 1 or x.shape[1] < 1)):
        raise ValueError("%s must have shape [T] or [B, T]%s, got %r" % (name, " with B, T >= 1" if strict else "", tuple(x.shape)))
    if x.dtype != torch.float32 and not (pcm16 and x.dtype == torch.int16):
        if strict:
            raise TypeError("%s must be float32, got %s" % (name, x.dtype))
        x = x.to(torch.float32)
    return x.to(device).contiguous()


def as_lengths(lengths, b, device):
    """``None``, or the ``b`` clips' own lengths as a contiguous device int64 ``[b]``."""
    import torch
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(device=device, dtype=torch.int64).contiguous()
    if tuple(lengths.shape) != (b,):
        raise ValueError("lengths must have shape [%d], got %r" % (b, tuple(lengths.shape)))
    return lengths
