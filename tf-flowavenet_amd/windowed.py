"""Windowed driving of a ``FloWaveNet`` (``model.py`` keeps the public methods and delegates here): clips of any length cut by
``windowing.plan_windows``, windows of equal length sharing one ``fwn_model_synthesize_windows`` / ``fwn_model_forward_windows`` /
``fwn_model_reverse`` call, and the two streams over ``windowing.StreamPlanner``.  Host sequencing only; the planning itself is
``windowing.py`` (no torch, no device).  ``model`` is the ``FloWaveNet``: it owns the library handle, the packed parameters and
the workspace cache (``_window_workspace``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, windowing


# ---------------------------------------------------------------------- the per-window tables of one group call
def upload_tables(cols64, cols32, device):
    """The per-window tables of one group call as ONE upload: ``cols64`` - the int64 columns - first, so that every column is
    aligned, then ``cols32`` - the 32-bit ones, integers in [-2^31, 2^32) kept mod 2^32 (int32 offsets and uint32 ids alike).
    Every column holds one value per window.  -> ``(buffer, pointers of cols64, pointers of cols32)``; the buffer is a uint8
    tensor on ``device`` that the caller keeps until the call is enqueued."""
    import torch
    t64 = np.asarray(cols64, dtype=np.int64).reshape(-1)
    t32 = np.asarray(cols32, dtype=np.int64).astype(np.uint32).reshape(-1)
    tab = torch.from_numpy(np.concatenate([t64.view(np.uint8), t32.view(np.uint8)])).to(device)
    n, p64 = (t64.size + t32.size) // max(1, len(cols64) + len(cols32)), tab.data_ptr()     # windows: every column's length
    assert p64 % 8 == 0
    return tab, [p64 + 8 * n * i for i in range(len(cols64))], [p64 + 8 * t64.size + 4 * n * i for i in range(len(cols32))]


def synthesize_windows_call(model, mel_flat, rows, length, seed, temp, pcm_flat, wav_flat):
    """One ``fwn_model_synthesize_windows`` group.  rows: per window ``(clip_id, start, mel_row, core_off, core_len, out_off)``
    - the window is samples [start, start + length) of clip ``clip_id``'s latent stream, its mel rows start at row
    ``mel_row`` of ``mel_flat``, and ``core_len`` samples from ``core_off`` of its waveform go to element ``out_off`` of
    ``pcm_flat`` (and ``wav_flat``)."""
    clip_id, start, mel_row, core_off, core_len, out_off = zip(*rows)
    tab, (p_start, p_mel, p_out), (p_id, p_off, p_len) = upload_tables([start, mel_row, out_off], [clip_id, core_off, core_len], model._device)
    wsp, wsn = model._window_workspace("synth", len(rows), length)
    rc = model._lib.fwn_model_synthesize_windows(C.byref(model._packed.model_desc), len(rows), length, mel_flat.data_ptr(), p_mel,
                                                 p_id, p_start, p_off, p_len, p_out, int(seed) % (1 << 64), float(temp), wsp, wsn,
                                                 pcm_flat.data_ptr(), None if wav_flat is None else wav_flat.data_ptr(), model._stream())
    _lib.check(rc, "fwn_model_synthesize_windows")


def forward_windows_call(model, x_flat, mel_flat, rows, length, acc, z_flat):
    """One ``fwn_model_forward_windows`` group.  rows: per window ``(x_row, mel_row, core_off, core_len, slot, z_off)`` - the
    window's audio starts at row ``x_row`` of ``x_flat`` (rows of hop samples), its mel at row ``mel_row`` of ``mel_flat``;
    the sums over ``core_len`` samples from ``core_off`` go to ``acc[slot]``, and that core of the latent, in time order, to
    element ``z_off`` of ``z_flat`` (None: no latent)."""
    x_row, mel_row, core_off, core_len, slot, z_off = zip(*rows)
    tab, (p_x, p_mel, p_z), (p_off, p_len, p_slot) = upload_tables([x_row, mel_row, z_off], [core_off, core_len, slot], model._device)
    wsp, wsn = model._window_workspace("forward", len(rows), length)
    rc = model._lib.fwn_model_forward_windows(C.byref(model._packed.model_desc), len(rows), length, x_flat.data_ptr(), p_x,
                                              mel_flat.data_ptr(), p_mel, p_off, p_len, p_slot, acc.data_ptr(), p_z,
                                              None if z_flat is None else z_flat.data_ptr(), wsp, wsn, model._stream())
    _lib.check(rc, "fwn_model_forward_windows")


def forward_windows_finish(model, acc, slot0, nwin):
    """``fwn_forward_windows_finish``: clip c's windows are slots ``slot0[c] .. slot0[c] + nwin[c]`` of ``acc`` -> fp32 [2, B]."""
    import torch
    b = len(slot0)
    tab, _, (p_slot0, p_nwin) = upload_tables([], [slot0, nwin], model._device)
    out = torch.empty(2, b, dtype=torch.float32, device=model._device)
    rc = model._lib.fwn_forward_windows_finish(acc.data_ptr(), p_slot0, p_nwin, b, out.data_ptr(), model._stream())
    _lib.check(rc, "fwn_forward_windows_finish")
    return out


# ---------------------------------------------------------------------- whole clips, group by group
def run_groups(model, plans, batch, row_of, call):
    """The windows of ``plans`` (one ``windowing.plan_windows`` list per clip), ``batch`` at a time: for every group of
    ``windowing.group_windows``, ``call([row_of(clip, k, lo, hi, a, e) for its windows], hi - lo)`` - one device call."""
    for group in windowing.group_windows(plans, batch, model._hparams):
        rows = [row_of(clip, k, *plans[clip][k]) for clip, k in group]
        lo, hi = plans[group[0][0]][group[0][1]][:2]
        call(rows, hi - lo)


def reverse_windowed(model, z, c, window, batch, halo, g):
    import torch
    model._check_g(g)
    b, t, z32, c32 = model._prep(z, c, "z")
    hop, dev = model.hop, model._device
    x = torch.empty(b, t, 1, dtype=torch.float32, device=dev)

    def call(spans, length):
        zg = torch.stack([z32[clip, lo:hi] for clip, lo, hi, _, _ in spans])
        cg = torch.stack([c32[clip, lo // hop:hi // hop] for clip, lo, hi, _, _ in spans])
        xg = torch.empty(len(spans), length, 1, dtype=torch.float32, device=dev)
        wsp, wsn = model._window_workspace("reverse", len(spans), length)
        rc = model._lib.fwn_model_reverse(C.byref(model._packed.model_desc), len(spans), length, zg.data_ptr(), cg.data_ptr(),
                                          wsp, wsn, xg.data_ptr(), model._stream())
        _lib.check(rc, "fwn_model_reverse")
        for row, (clip, lo, _, a, e) in enumerate(spans):
            x[clip, a:e] = xg[row, a - lo:e - lo]

    run_groups(model, [windowing.plan_windows(t, window, model._hparams, halo)] * b, batch, lambda clip, k, *span: (clip,) + span, call)
    return x


def synthesize_windowed(model, c, seed, clip_ids, window, batch, temp, return_wav, halo):
    import torch
    model._require_params()
    model._check_c(c)
    hp, hop, dev = model._hparams, model.hop, model._device
    temp = float(hp.temp if temp is None else temp)
    b, frames = int(c.shape[0]), int(c.shape[1])
    t = frames * hop
    if b < 1:
        raise ValueError("c holds no clip")
    if t > (1 << 34):
        raise ValueError("T=%d exceeds the 2^34 samples one clip's latent stream numbers" % t)
    plans = [windowing.plan_windows(t, window, hp, halo)] * b
    ids = list(range(b)) if clip_ids is None else model._clip_id_values(clip_ids, b)
    c32 = c.to(device=torch.device(dev), dtype=torch.float32).contiguous()
    pcm = torch.empty(b, t, dtype=torch.int16, device=dev)
    wav = torch.empty(b, t, 1, dtype=torch.float32, device=dev) if return_wav else None
    run_groups(model, plans, batch,
               lambda clip, k, lo, hi, a, e: (ids[clip], lo, clip * frames + lo // hop, a - lo, e - a, clip * t + a),
               lambda rows, length: model._windows_call(c32, rows, length, seed, temp, pcm, wav))
    return (pcm, wav) if return_wav else pcm


def check_forward(model):
    model._require_params()
    if model._gate_fp8:
        raise ValueError("a gate_fp8 model takes no windows: the windowed forward runs the ragged forward's form of the pass")
    if model._init:
        raise ValueError("init=True takes no windows: the data-dependent ActNorm init needs the moments of the whole batch")


def forward_windowed(model, x, c, window, batch, return_z, halo, g):
    import torch
    model._check_g(g)
    check_forward(model)
    b, t, x32, c32 = model._prep(x, c, "x")
    if t > (1 << 34):
        raise ValueError("T=%d exceeds 2^34 samples per clip" % t)
    hp, hop, dev = model._hparams, model.hop, model._device
    plan = windowing.plan_windows(t, window, hp, halo)
    nwin, frames = len(plan), t // hop
    acc = torch.zeros(b * nwin, 4, dtype=torch.float64, device=dev)
    z = torch.empty(b, t, 1, dtype=torch.float32, device=dev) if return_z else None
    run_groups(model, [plan] * b, batch,
               lambda clip, k, lo, hi, a, e: (clip * frames + lo // hop, clip * frames + lo // hop, a - lo, e - a, clip * nwin + k,
                                              clip * t + a),
               lambda rows, length: model._forward_windows_call(x32, c32, rows, length, acc, z))
    out = model._forward_windows_finish(acc, [clip * nwin for clip in range(b)], [nwin] * b)
    return (out[0], out[1], z) if return_z else (out[0], out[1])


# ---------------------------------------------------------------------- one clip that is still arriving
def _grown(buf, used, need, like):
    """``buf`` with room for ``need`` rows (doubling), its first ``used`` rows kept; ``like``: a tensor of the row's shape and dtype."""
    import torch
    if buf is not None and need <= buf.shape[0]:
        return buf
    grown = torch.empty((max(need, 2 * (0 if buf is None else buf.shape[0])),) + tuple(like.shape[1:]), dtype=like.dtype,
                        device=like.device)
    if used:
        grown[:used] = buf[:used]
    return grown


class _WindowStream:
    """What both streams are: a ``windowing.StreamPlanner`` and, on the device, the rows of frames ``_base .. _base + _n`` of the
    clip, one buffer per kind of row (``_bufs``, grown by doubling).  ``_push`` appends a push's rows and runs the windows that
    became computable; after each run the frames no later window reads are dropped.  A stream supplies what one frame's rows
    are (its ``push``), ``_window(lo, hi, a, e, row)`` - the device call of one window whose first frame is row ``row`` of the
    buffers, -> its output or None - and what ``finish`` adds; ``_dtype`` names the output's type."""

    def __init__(self, model, window, halo, nbuf):
        self._model = model
        self._plan = windowing.StreamPlanner(model._hparams, window, halo)
        self._bufs = [None] * nbuf
        self._base = 0
        self._n = 0

    @property
    def retained_frames(self):
        return self._n

    def _mel_rows(self, frames, name):
        import torch
        m = self._model
        f = torch.as_tensor(frames).to(device=torch.device(m._device), dtype=torch.float32)
        if f.dim() != 2 or f.shape[1] != m._hparams.num_mels:
            raise ValueError("%s must have shape [f, %d], got %r" % (name, m._hparams.num_mels, tuple(f.shape)))
        return f

    def _push(self, *parts):
        """parts: the push's rows, one [f, width] tensor per buffer."""
        need = self._n + int(parts[0].shape[0])
        for i, part in enumerate(parts):
            self._bufs[i] = _grown(self._bufs[i], self._n, need, part)
            self._bufs[i][self._n:need] = part
        new, self._n = need - self._n, need
        return self._run(self._plan.push(new))

    def _run(self, windows):
        import torch
        m = self._model
        out = [self._window(lo, hi, a, e, lo // m.hop - self._base) for lo, hi, a, e in windows]
        out = [o for o in out if o is not None]
        drop = min(self._plan.first_frame - self._base, self._n)      # frames no later window reads
        if drop > 0:
            for buf in self._bufs:
                buf[:self._n - drop] = buf[drop:self._n].clone()
            self._base, self._n = self._base + drop, self._n - drop
        if not out:
            return torch.empty(0, dtype=getattr(torch, self._dtype), device=m._device)
        return out[0] if len(out) == 1 else torch.cat(out)

    def finish(self):
        return self._run(self._plan.finish())


class SynthesisStream(_WindowStream):
    """``FloWaveNet.stream``: 16-bit PCM of one clip while its mel is still arriving.  ``push(frames)`` takes [f, num_mels] (a
    tensor or an array, any f >= 0) and returns the PCM of the cores that became computable with them, one ``torch.int16``
    tensor on the device, possibly empty; ``finish()`` returns the rest (``ValueError`` if the frame total is no multiple of
    lcm(hop_size, 2^n_block) / hop_size).  One ``fwn_model_synthesize_windows`` call per window; the object keeps only the
    mel frames a later window still needs - at most (window + 2 H) / hop plus one push (``windowing.StreamPlanner``)."""
    _dtype = "int16"

    def __init__(self, model, seed, clip_id=0, window=None, temp=None, halo=None):
        super().__init__(model, window, halo, 1)     # [capacity, num_mels]
        self._seed = int(seed)
        self._clip = model._clip_id_values([clip_id], 1)[0]
        self._temp = float(model._hparams.temp if temp is None else temp)

    def push(self, frames):
        return self._push(self._mel_rows(frames, "frames"))

    def _window(self, lo, hi, a, e, row):
        import torch
        pcm = torch.empty(e - a, dtype=torch.int16, device=self._model._device)
        self._model._windows_call(self._bufs[0], [(self._clip, lo, row, a - lo, e - a, 0)], hi - lo, self._seed, self._temp, pcm, None)
        return pcm


class ForwardStream(_WindowStream):
    """``FloWaveNet.forward_stream``: log_p, logdet and the time-ordered latent of one clip while it is still arriving - the twin
    of ``SynthesisStream`` over the same ``windowing.StreamPlanner``.  ``push(x_samples, c_frames)`` takes f * hop samples (any
    shape holding that many) and their f mel frames [f, num_mels] (tensors or arrays, any f >= 0) and returns the z of the cores
    that became computable, one fp32 tensor on the device, possibly empty (always empty without ``return_z``); ``finish()``
    returns ``(z_rest, log_p, logdet)``, the scalars fp32 0-dim tensors (``ValueError`` if the frame total is no multiple of
    lcm(hop_size, 2^n_block) / hop_size, or nothing was pushed).  One ``fwn_model_forward_windows`` call per window; window k's
    sums wait in slot k of a device table until ``finish`` adds them in window order.  The object keeps only the audio and mel
    a later window still needs - at most (window + 2 H) / hop frames plus one push."""
    _dtype = "float32"

    def __init__(self, model, window=None, halo=None, return_z=True):
        super().__init__(model, window, halo, 2)     # [capacity, hop] audio, [capacity, num_mels] mel
        self._return_z = bool(return_z)
        self._acc = None             # device [capacity, 4] fp64: window k's partial sums in row k
        self._k = 0                  # windows run

    def push(self, x_samples, c_frames):
        import torch
        hop = self._model.hop
        f = self._mel_rows(c_frames, "c_frames")
        xs = torch.as_tensor(x_samples).to(device=f.device, dtype=torch.float32).reshape(-1)
        if xs.numel() != int(f.shape[0]) * hop:
            raise ValueError("%d frames go with %d samples (hop_size=%d), got %d" % (f.shape[0], f.shape[0] * hop, hop, xs.numel()))
        return self._push(xs.reshape(-1, hop), f)

    def _window(self, lo, hi, a, e, row):
        import torch
        dev = self._model._device
        z = torch.empty(e - a, dtype=torch.float32, device=dev) if self._return_z else None
        if self._acc is None or self._k == self._acc.shape[0]:
            self._acc = _grown(self._acc, self._k, self._k + 1, torch.empty(1, 4, dtype=torch.float64, device=dev))
        self._model._forward_windows_call(self._bufs[0], self._bufs[1], [(row, row, a - lo, e - a, self._k, 0)], hi - lo, self._acc, z)
        self._k += 1
        return z

    def finish(self):
        rest = super().finish()
        if not self._k:
            raise ValueError("finish: nothing was pushed")
        out = self._model._forward_windows_finish(self._acc, [0], [self._k])
        return rest, out[0, 0], out[1, 0]
