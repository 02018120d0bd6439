"""Host planning of windowed synthesis (``FloWaveNet.reverse_windowed`` / ``synthesize_windowed`` / ``stream``): pure Python,
no device, no torch.

The network is fully convolutional with a finite receptive field, so a long clip can be cut into windows,
each run through the ordinary inverse pass with enough real context - a halo - on both sides, and only the cores kept.
``halo_samples`` is the halo that makes the kept samples those of the whole-clip pass exactly (tests/test_windowed_host.py holds
it to the fp64 oracle at 1e-12):

    R    = 1 + sum_{l < n_layer} 3^l                     one WaveNet's reach in rows: the front conv plus the dilations
    unit = lcm(hop_size, 2^n_block)
    H    = n_flow * R * (2^(n_block+1) - 2) + 2 * hop_size, rounded up to a multiple of unit

The first term is the flows' reach in samples from a cut at a multiple of 2^n_block (a row of block i is 2^(i+1) samples,
n_flow WaveNets per block); the second the two mel frames whose up-sampled rows the transposed convolutions get wrong next to
a cut.
"""
from __future__ import annotations

import math


def unit_samples(hparams):
    """lcm(hop_size, 2^n_block): what every window edge is a multiple of."""
    return math.lcm(int(hparams.hop_size), 1 << int(hparams.n_block))


def round_up_to_unit(samples, hparams):
    """``samples`` rounded up to a multiple of ``unit_samples``."""
    unit = unit_samples(hparams)
    return -(-int(samples) // unit) * unit


def default_window(hparams):
    """The window of every windowed entry that is given none: 65 536 samples, rounded up to the unit."""
    return round_up_to_unit(65536, hparams)


def halo_samples(hparams):
    """The halo H in samples (module docstring): 15 872 for the stock model, 2 112 for ``hparams8000``."""
    reach = 1 + sum(3 ** layer for layer in range(int(hparams.n_layer)))
    h = int(hparams.n_flow) * reach * ((2 << int(hparams.n_block)) - 2) + 2 * int(hparams.hop_size)
    return round_up_to_unit(h, hparams)


def _check_window(window, halo, hparams):
    unit = unit_samples(hparams)
    if window is None:
        window = default_window(hparams)
    if int(window) != window or window < unit or window % unit:
        raise ValueError("window=%r must be a positive multiple of lcm(hop_size, 2^n_block) = %d" % (window, unit))
    if halo is None:
        return int(window), halo_samples(hparams), unit
    if int(halo) != halo or halo < 0 or halo % unit:
        raise ValueError("halo=%r must be a non-negative multiple of lcm(hop_size, 2^n_block) = %d" % (halo, unit))
    return int(window), int(halo), unit


def plan_windows(t, window, hparams, halo=None):
    """The windows of a clip of ``t`` samples: a list of ``(lo, hi, a, b)`` in samples.  The cores ``[a, b)`` tile ``[0, t)`` in
    order in steps of ``window`` (the last one may be shorter); window k is ``[lo, hi) = [max(0, a - H), min(t, b + H))`` - the
    inverse pass runs on that, and ``[a - lo, b - lo)`` of its output is kept.  ``window`` is a positive multiple of
    ``unit_samples`` (None, here and in ``StreamPlanner``: ``default_window``), ``t`` a multiple of it; ``halo`` (a multiple
    of it too) overrides ``halo_samples`` - 0 is the cut without context, the negative control of the tests.  A clip with
    ``t <= window`` is one window and needs no halo."""
    window, h, unit = _check_window(window, halo, hparams)
    if int(t) != t or t < unit or t % unit:
        raise ValueError("t=%r must be a positive multiple of lcm(hop_size, 2^n_block) = %d" % (t, unit))
    t = int(t)
    return [(max(0, a - h), min(t, min(t, a + window) + h), a, min(t, a + window)) for a in range(0, t, window)]


def max_windows_per_call(hparams, length):
    """How many windows of ``length`` samples one inverse pass may take: every activation buffer is addressed with 32-bit
    offsets below 2 GiB (``synthesize.max_clips_per_call``'s rule; csrc/api.hip check_model)."""
    lim = min(((1 << 31) - 1) // (int(hparams.n_layer) * 256), ((1 << 31) - 1) // int(hparams.num_mels))
    return int((lim - 1) // int(length))


def group_windows(plans, batch, hparams=None):
    """Which windows share a call.  ``plans``: one ``plan_windows`` list per clip.  -> a list of groups, each a list of ``(clip,
    k)`` (window k of clip ``clip``): windows of equal length ``hi - lo`` share a call, up to ``batch`` of them - with
    ``hparams`` given, up to ``max_windows_per_call`` if that is fewer - the windows of all clips pooled: every call is a
    plain rectangular inverse pass.  Lengths come in order of first appearance, windows in (clip, k) order inside a length; a
    long clip cut at a window of at least the halo has at most four lengths (first, middle, and one or two at the end)."""
    if int(batch) != batch or batch < 1:
        raise ValueError("batch=%r must be a positive integer" % (batch,))
    by_len = {}
    for clip, plan in enumerate(plans):
        for k, (lo, hi, _, _) in enumerate(plan):
            by_len.setdefault(hi - lo, []).append((clip, k))
    groups = []
    for length, members in by_len.items():
        per_call = int(batch) if hparams is None else min(int(batch), max_windows_per_call(hparams, length))
        if per_call < 1:
            raise ValueError("a window of %d samples (halo included) exceeds what one call can address (%d samples): use a "
                             "smaller window" % (length, max_windows_per_call(hparams, 1)))
        groups += [members[i:i + per_call] for i in range(0, len(members), per_call)]
    return groups


class StreamPlanner:
    """The windows of a clip whose mel arrives frame by frame - the bookkeeping of ``FloWaveNet.stream`` without the device.

    ``push(f)`` takes the number of new frames and returns the windows ``(lo, hi, a, b)`` that became computable: core k =
    ``[k window, (k+1) window)`` is released as soon as ``(b_k + H) / hop`` frames have arrived, whatever the split into pushes.
    ``finish()`` releases the rest, clamped to the clip's end - together exactly ``plan_windows(total, window)`` - and raises
    ``ValueError`` if the total is no multiple of ``unit / hop`` frames.  ``first_frame`` is the earliest frame a later window
    still needs: everything before it may be dropped, so the retained frames never exceed ``(window + 2 H) / hop`` plus one push."""

    def __init__(self, hparams, window, halo=None):
        self.window, self.halo, self.unit = _check_window(window, halo, hparams)
        self.hop = int(hparams.hop_size)
        self.frames = 0          # frames arrived
        self.next_core = 0       # the first core not yet released
        self.done = False

    @property
    def first_frame(self):
        return max(0, self.next_core * self.window - self.halo) // self.hop

    def push(self, f):
        if self.done:
            raise ValueError("push after finish")
        if int(f) != f or f < 0:
            raise ValueError("a push holds a non-negative number of frames, got %r" % (f,))
        self.frames += int(f)
        out = []
        while ((self.next_core + 1) * self.window + self.halo) <= self.frames * self.hop:
            a = self.next_core * self.window
            out.append((max(0, a - self.halo), a + self.window + self.halo, a, a + self.window))
            self.next_core += 1
        return out

    def finish(self):
        if self.done:
            raise ValueError("finish called twice")
        t = self.frames * self.hop
        if t % self.unit:
            raise ValueError("%d frames in all: the total must be a multiple of %d frames (lcm(hop_size, 2^n_block) = %d samples)"
                             % (self.frames, self.unit // self.hop, self.unit))
        self.done = True
        out = []
        for a in range(self.next_core * self.window, t, self.window):
            b = min(t, a + self.window)
            out.append((max(0, a - self.halo), min(t, b + self.halo), a, b))
            self.next_core += 1
        return out
