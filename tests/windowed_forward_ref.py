"""The fp64 composition behind the windowed forward's tests (no GPU): the oracle's forward pass rebuilt from its own functions
(``upsample``, ``squeeze``, ``actnorm_forward``, ``wavenet``, ... - the way tests/test_ragged_init.py composes them) so that
every flow's ``log_s`` stays available, and from it the per-window CORE sums and the rule that adds them up per clip:

    log_p  = 0.5 (-log 2 pi - sum_windows sum_core z^2 / t)
    logdet = sum_flows mean_C(3 logs) + sum_windows sum_flows sum_{core rows, c}(-log_s) / t

A flow of block i has t / 2^(i+1) rows of 2^i log_s channels: t / 2 elements, so the reference's mean(-log_s) / 2 is
sum(-log_s) / t at every block.  Core edges are multiples of lcm(hop, 2^n_block): whole rows at every block."""
import math

import numpy as np

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd import windowing as WIN


def time_order(out, n_block):
    """The reference's final ``out`` [B, T / 2^n, 2^n] un-squeezed n_block times -> [B, T]: what ``reverse`` takes."""
    for _ in range(n_block):
        out = onp.unsqueeze(out)
    return out[:, :, 0]


def forward_terms(p, x, c, hp):
    """The forward pass of x [1, T, 1], c [1, T / hop, num_mels] in the arrays' own precision -> (z_time [T], log_s: one array
    [rows, Ch] per flow in (block, flow) order, actnorm: sum over the flows of mean_C(3 logs))."""
    out, cond = x, onp.upsample(p, c, hp)
    log_s_all, actnorm = [], 0.0
    for i in range(hp.n_block):
        out, cond = onp.squeeze(out), onp.squeeze(cond)
        for j in range(hp.n_flow):
            prefix = "Block_%d/Flow_%d" % (i, j)
            out, an = onp.actnorm_forward(p, prefix + "/ActNorm", out)
            in_a, in_b = onp.split2(out)
            net = onp.wavenet(p, prefix + "/WaveNet", in_a, onp.split2(cond)[0], hp.n_layer, hp.causality)
            log_s, t = onp.split2(net)
            out = np.concatenate([in_a, (in_b - t) * np.exp(-log_s)], 2)
            out, cond = onp.change_order(out, cond)
            log_s_all.append(log_s[0])
            actnorm += float(an)
    return time_order(out, hp.n_block)[0], log_s_all, actnorm


def windowed_forward(p, x, c, hp, window, halo=None):
    """The fp64 statement of ``FloWaveNet.forward_windowed`` for one clip: x [T], c [T / hop, num_mels] -> (log_p, logdet, z_time
    [T]) from the windows of ``plan_windows`` - each run through ``forward_terms`` on its own, only its core kept."""
    t = len(x)
    z = np.full(t, np.nan)
    z2 = ls = 0.0
    actnorm = None
    for lo, hi, a, b in WIN.plan_windows(t, window, hp, halo):
        zw, log_s, an = forward_terms(p, x[None, lo:hi, None], c[None, lo // hp.hop_size:hi // hp.hop_size], hp)
        z[a:b] = zw[a - lo:b - lo]
        z2 += float(np.square(zw[a - lo:b - lo]).sum())
        for f, s in enumerate(log_s):
            shift = f // hp.n_flow + 1                  # a row of block i is 2^(i+1) samples
            ls += float(-s[(a - lo) >> shift:(b - lo) >> shift].sum())
        actnorm = an if actnorm is None else actnorm     # the same for every window
    return 0.5 * (-math.log(2.0 * math.pi) - z2 / t), actnorm + ls / t, z


_CASES = {}


def oracle_case(cfg, units):
    """Once per geometry of tests/test_windowed_host.py, never changed: one clip's x and c (float32 [1, ...], as a model takes
    them), the loud parameters, the fp64 oracle's whole-clip forward (log_p, logdet, z in time order), and the fp64 windowed
    composition with the halo and with none.  tests/test_windowed_forward.py holds the GPU paths to the same arrays."""
    from test_windowed_host import case_shape, hp_of, loud_params
    key = repr(cfg)
    if key not in _CASES:
        hp = hp_of(cfg)
        t, window = case_shape(hp, units)
        params = loud_params(hp)
        p64 = onp.to_f64(params)
        inp = W.synthetic_inputs(hp, 1, t, want=("c", "x"))
        x, c = inp["x"].astype(np.float32), inp["c"].astype(np.float32)
        lp, ld, out = onp.forward(p64, x.astype(np.float64), c.astype(np.float64), hp)
        x64, c64 = x[0, :, 0].astype(np.float64), c[0].astype(np.float64)
        _CASES[key] = dict(hp=hp, t=t, window=window, params=params, p64=p64, x=x, c=c, log_p=lp, logdet=ld,
                           z=time_order(out, hp.n_block)[0], halo=windowed_forward(p64, x64, c64, hp, window),
                           cut=windowed_forward(p64, x64, c64, hp, window, halo=0))
    return _CASES[key]
