"""Spectral distances of synthesized audio against its target, on the device (csrc/specdist.hip):

    sd = SpectralDistance(hparams, resolutions=[(512, 128), (1024, 256), (2048, 512)])
    d = sd.dist(target, test, lengths=None)          # float32 [T] or [B, T] on the device
    d["mel_l1"], d["lsd_db"], d["sc"], d["frames"]   # float64 [B] on the device

``mel_l1`` is the mean absolute difference of the two clips' log-mels - ``MelFrontEnd(normalize=False)``'s, bit for bit - at
the model's own ``(n_fft, hop_size)``, whatever ``resolutions`` says; ``lsd_db`` (log-spectral distance, dB) and ``sc`` (spectral
convergence) are the means over ``resolutions`` (default: the model's own, alone) and come per resolution under
``"lsd_db@1024/256"``-style keys as well; ``frames`` counts the model-resolution frames.  No spectrogram is written to memory
and nothing comes down: a call is two launches per resolution, and a clip's numbers do not depend on its batch.  A clip shorter
than ``n_fft / 2 + 1`` samples at some resolution gets NaN there.  There is no CPU fallback.
"""
from __future__ import annotations

from . import _lib
from .preprocessing import mel_bands, mel_filterbank
from .rows import as_lengths, as_rows, check_shape

MEASURES = ("mel_l1", "lsd_db", "sc")


def resolution_arg(text):
    """``"512/128,1024/256"`` -> [(512, 128), (1024, 256)] (the CLI's ``--resolutions``)."""
    out = []
    for part in str(text).split(","):
        n_fft, sep, hop = part.partition("/")
        if not sep:
            raise ValueError("a resolution is n_fft/hop, got %r" % part)
        out.append(check_shape(int(n_fft), int(hop)))
    return out


def key_of(name, n_fft, hop):
    return "%s@%d/%d" % (name, n_fft, hop)


def combine(per_res, own, resolutions, mean=None):
    """The result dict from the ``[B, 4]`` blocks (mel_l1, lsd_db, sc, frames): ``own`` at the model's resolution, ``per_res``
    one per entry of ``resolutions``.  ``mean``: the mean of a list of ``[B]`` columns (default: summed in order, divided)."""
    if mean is None:
        def mean(cols):
            s = cols[0]
            for c in cols[1:]:
                s = s + c
            return s / float(len(cols))
    out = {"mel_l1": own[:, 0], "frames": own[:, 3],
           "lsd_db": mean([r[:, 1] for r in per_res]), "sc": mean([r[:, 2] for r in per_res])}
    for (n_fft, hop), r in zip(resolutions, per_res):
        out[key_of("lsd_db", n_fft, hop)] = r[:, 1]
        out[key_of("sc", n_fft, hop)] = r[:, 2]
    return out


class SpectralDistance:
    """See the module's text.  ``floor`` is the power floor of ``lsd_db`` (default 1e-4, the front-end's own)."""

    def __init__(self, hparams, resolutions=None, floor=1e-4, device="cuda"):
        import torch
        self._hp = hparams
        self.own = check_shape(hparams.n_fft, hparams.hop_size)
        self.resolutions = [self.own] if resolutions is None else [check_shape(n, h) for n, h in resolutions]
        if not self.resolutions:
            raise ValueError("resolutions must not be empty")
        self.floor = float(floor)
        if not (self.floor > 0.0 and self.floor < float("inf")):
            raise ValueError("floor must be a finite positive power, got %r" % (floor,))
        self._lib = _lib.load()          # fails loudly when libfwn.so is missing
        self._device = torch.device(device)
        fb = mel_filterbank(hparams)
        self._fb = torch.from_numpy(fb).to(self._device)
        self._bands = torch.from_numpy(mel_bands(fb)).to(self._device)
        self._ws = {}                    # (B, T, n_fft, hop, stream) -> workspace

    def _workspace(self, b, t, n_fft, hop, stream):
        import torch
        key = (b, t, n_fft, hop, stream)
        if key not in self._ws:
            while len(self._ws) >= 16:
                del self._ws[next(iter(self._ws))]
            n = int(self._lib.fwn_spectral_distance_workspace_bytes(b, t, n_fft, hop))
            self._ws[key] = torch.empty(max(n, 8) // 8, dtype=torch.float64, device=self._device)
        return self._ws[key]

    def one(self, x, y, lengths, n_fft, hop, mel):
        """One resolution: device float64 ``[B, 4]`` = mel_l1 (NaN unless ``mel``), lsd_db, sc, frames.  x, y: ``as_rows``."""
        import torch
        hp = self._hp
        b, t = int(x.shape[0]), int(x.shape[1])
        stream = torch.cuda.current_stream(self._device).cuda_stream
        ws = self._workspace(b, t, n_fft, hop, stream)
        out = torch.empty(b, 4, dtype=torch.float64, device=self._device)
        rc = self._lib.fwn_spectral_distance(x.data_ptr(), t, y.data_ptr(), t, b, None if lengths is None else lengths.data_ptr(), t,
                                             self._fb.data_ptr() if mel else None, self._bands.data_ptr() if mel else None, n_fft, hop,
                                             hp.num_mels, float(hp.ref_level_db), float(hp.min_level_db), self.floor, out.data_ptr(),
                                             ws.data_ptr(), ws.numel() * 8, stream)
        _lib.check(rc, "fwn_spectral_distance")
        return out

    def dist(self, ref, test, lengths=None):
        x, y = as_rows(ref, "ref", self._device, strict=True), as_rows(test, "test", self._device, strict=True)
        if x.shape != y.shape:
            raise ValueError("ref %r and test %r differ in shape" % (tuple(x.shape), tuple(y.shape)))
        lengths = as_lengths(lengths, int(x.shape[0]), self._device)
        own = self.one(x, y, lengths, self.own[0], self.own[1], True)
        per_res = [own if r == self.own else self.one(x, y, lengths, r[0], r[1], False) for r in self.resolutions]
        return combine(per_res, own, self.resolutions)
