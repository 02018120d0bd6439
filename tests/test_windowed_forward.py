"""Windowed forward on the GPU (-m gpu): the kernels around the pass against fp64 NumPy and, for the latent, bit for bit against
what they restate; ``forward_windowed`` / ``forward_stream`` against the fp64 oracle's WHOLE-clip forward; ``score --window``.

What is held to what.  That the halo is exact, and that per-clip scalars composed from core sums are the whole clip's, is proved
in fp64 on the CPU (tests/test_windowed_forward_host.py: 1e-12).  These tests catch what the device path adds: row ranges,
offsets, slots, seams.  Bounds: tests/test_ragged_forward.py's, copied - ``REL_LOGP``, ``ABS_LOGDET``, ``ABS_Z``, ``ABS_WAV``.  The
latent is held at the loud weights of the fp64 proof (``ABS_Z max(1, |z|max)``; the same call with ``halo=0`` must EXCEED it -
the control: these tests see a seam), the scalars at the stock weights ``W.synthetic_params(hp, 99, actnorm="random")``, where
tests/test_ragged_forward.py holds its scalars.  Sums: 1e-6 relative of the fp64 NumPy sum (fp32 inputs, fp64 accumulation in
another order); copies bit for bit; repeated calls bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_windowed_host as H  # noqa: E402
import windowed_forward_ref as R  # noqa: E402
from test_windowed import _i32, _i64, dev  # noqa: E402

from oracle import flowavenet_np as onp  # noqa: E402
from tf_flowavenet_amd import _lib  # noqa: E402
from tf_flowavenet_amd import weights as W  # noqa: E402
from tf_flowavenet_amd import windowing as WIN  # noqa: E402
from tf_flowavenet_amd.model import FloWaveNet, z_planes_to_squeezed  # noqa: E402

from conftest import small_hparams  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_LOGP = 1e-3
ABS_LOGDET = 1e-3
ABS_Z = 2e-2
ABS_WAV = 1e-2
Z_MEAN, Z_P9999, Z_MAX = 2.5e-3, 1.5e-2, 2.5e-2     # tests/test_gpu_parity.py's full-size latent statistics


def check_scalars(log_p, logdet, lp0, ld0):
    print("log_p %.6f (oracle %.6f)  logdet %.6f (oracle %.6f)" % (float(log_p), lp0, float(logdet), ld0))
    assert abs(float(log_p) - lp0) <= REL_LOGP * abs(lp0), (float(log_p), lp0)
    assert abs(float(logdet) - ld0) <= ABS_LOGDET * max(1.0, abs(ld0)), (float(logdet), ld0)


def _clamp(off, n, size):
    off = min(max(off, 0), size)
    return off, min(max(n, 0), size - off)


# ---- 1. the two reductions alone ------------------------------------------------------------------------------------------
def _logdet_case(lib, rows, ch, cores, offset=0):
    """cores: (first row, rows) per window, handed over in samples; NaN in every row outside the core and in the t half of
    every row: a finite sum shows that nothing else entered it."""
    n, spr = len(cores), 2 * ch
    rng = np.random.default_rng(rows * 17 + ch)
    z = rng.standard_normal((n, rows, 2 * ch)).astype(np.float32)
    npt = max(1, ch // 32)
    ez = rng.uniform(0.5, 2.0, size=npt * 64).astype(np.float32)
    an = rng.standard_normal((2, 4, ch)).astype(np.float32)
    z[:, :, ch:] = np.nan
    want, mag = [], []
    tau = np.arange(ch)
    scale = ez[(tau // 32) * 64 + tau % 32].astype(np.float64)
    for k, (r0, nr) in enumerate(cores):
        r0, nr = _clamp(r0, nr, rows)
        z[k, :r0] = np.nan
        z[k, r0 + nr:] = np.nan
        body = z[k, r0:r0 + nr, :ch].astype(np.float64) * scale
        want.append(-body.sum())
        mag.append(np.abs(body).sum())
    nslot = lib.fwn_ragged_logdet_slots(n)
    zd = dev(np.concatenate([np.full(offset, np.nan, dtype=np.float32), z.reshape(-1), np.full(64, np.nan, dtype=np.float32)]))
    acc = torch.full((n, nslot), float("nan"), dtype=torch.float64, device="cuda")
    off_d, len_d = _i32(r0 * spr for r0, _ in cores), _i32(nr * spr for _, nr in cores)
    ezd, and_ = dev(ez), dev(an)
    outs = []
    for _ in range(2):
        rc = lib.fwn_window_logdet_rows(zd.data_ptr() + 4 * offset, n, rows, ch, ezd.data_ptr(), and_.data_ptr(), off_d.data_ptr(),
                                        len_d.data_ptr(), spr, acc.data_ptr(), None)
        assert rc == 0, lib.fwn_last_error()
        outs.append(acc.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])                                    # fixed-order sums: the same bits again
    got = outs[0]
    assert np.isfinite(got).all(), (rows, ch, cores, offset)
    for k in range(n):
        s = float(got[k, :nslot - 1].sum())
        assert abs(s - want[k]) <= 1e-6 * max(mag[k], 1e-30), (rows, ch, k, cores[k], s, want[k])
        a = float((an[0, 3].astype(np.float64) + an[1, 3].astype(np.float64)).sum())
        assert abs(float(got[k, nslot - 1]) - a) <= 1e-12 * max(1.0, float(np.abs(an[:, 3]).sum()))


def test_window_logdet_kernel_alone():
    lib = _lib.load()
    rows = 37
    # from row 0, a middle range, up to the last row, one-row cores (first, odd, even, last), everything, nothing, and tables
    # that must be clamped (a start before the buffer, a count past its end, a start past its end)
    cores = [(0, 9), (11, 13), (30, 7), (0, 1), (17, 1), (18, 1), (36, 1), (0, 37), (5, 0), (-3, 6), (33, 100), (50, 4)]
    for ch in (1, 2, 4, 16, 128):
        _logdet_case(lib, rows, ch, cores)
    _logdet_case(lib, 70001, 1, [(1, 70000), (0, 70001), (35001, 3), (2, 69997)])        # many chunks; Ch = 1 pairs rows: odd starts and ends
    _logdet_case(lib, 33333, 2, [(1, 33332), (16000, 9001), (33332, 1)])
    _logdet_case(lib, 3000, 64, [(1, 2999), (1500, 1499)])
    for ch in (1, 2, 4):                                                       # a base that is not 16-byte aligned
        _logdet_case(lib, 41, ch, [(0, 41), (7, 9), (40, 1), (3, 0)], offset=1)


def _both_entries_case(lib, nclip, rows, ch, lens):
    """``fwn_ragged_logdet_rows(lens)`` and ``fwn_window_logdet_rows(core_off = 0, core_len = lens)`` on the same Z, NaN past each
    clip's rows (and in the t half of every row): finite accumulators show that nothing outside the range was loaded, equal
    ones that the two entries add the same terms in the same order."""
    spr = 2 * ch
    rng = np.random.default_rng(rows * 19 + ch)
    z = rng.standard_normal((nclip, rows, 2 * ch)).astype(np.float32)
    z[:, :, ch:] = np.nan
    for k, n in enumerate(lens):
        z[k, min(max(n, 0) // spr, rows):] = np.nan
    ez = dev(rng.uniform(0.5, 2.0, size=max(1, ch // 32) * 64).astype(np.float32))
    an = dev(rng.standard_normal((2, 4, ch)).astype(np.float32))
    zd = dev(np.concatenate([z.reshape(-1), np.full(64, np.nan, dtype=np.float32)]))
    assert zd.data_ptr() % 16 == 0
    nslot = lib.fwn_ragged_logdet_slots(nclip)
    len_d, zero_d = _i32(lens), _i32([0] * nclip)
    got = []
    for start in (None, zero_d.data_ptr()):
        acc = torch.full((nclip, nslot), float("nan"), dtype=torch.float64, device="cuda")
        if start is None:
            rc = lib.fwn_ragged_logdet_rows(zd.data_ptr(), nclip, rows, ch, ez.data_ptr(), an.data_ptr(), len_d.data_ptr(), spr,
                                            acc.data_ptr(), None)
        else:
            rc = lib.fwn_window_logdet_rows(zd.data_ptr(), nclip, rows, ch, ez.data_ptr(), an.data_ptr(), start, len_d.data_ptr(), spr,
                                            acc.data_ptr(), None)
        assert rc == 0, lib.fwn_last_error()
        got.append(acc.cpu().numpy())
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), (nclip, rows, ch, lens)
    assert np.array_equal(got[0], got[1]), (nclip, rows, ch, lens)             # the ActNorm slot included


def test_ragged_and_window_entries_leave_the_same_sums():
    """The shapes of ``test_ragged_logdet_kernel_alone`` (tests/test_ragged_forward.py) from a 16-byte-aligned buffer: all four
    load branches, several chunks per clip.  At Ch = 1 a row is 8 bytes and both row counts are odd, so in a batch every other
    clip starts 8 bytes off; each of those clips therefore also goes through both entries alone, from the buffer's base."""
    lib = _lib.load()
    rows = 37
    for ch in (1, 2, 4, 16, 128):
        spr = 2 * ch
        lens = [0, rows * spr, rows * spr + 1000, spr, (rows - 1) * spr, -5]
        _both_entries_case(lib, 6, rows, ch, lens)
        if ch == 1:
            for n in lens:
                _both_entries_case(lib, 1, rows, ch, [n])
    _both_entries_case(lib, 3, 70001, 1, [2, 140002, 70000])                   # many chunks per clip, odd rows (Ch = 1 pairs rows)
    for n in (2, 140002, 70000):
        _both_entries_case(lib, 1, 70001, 1, [n])


def _sums_case(lib, length, cores, slots, nflows, n_flow, offset=0):
    n, half = len(cores), length // 2
    rng = np.random.default_rng(length * 7 + nflows)
    planes = rng.standard_normal((2, n, half)).astype(np.float32)
    nslot = lib.fwn_ragged_logdet_slots(n)
    acc = rng.standard_normal((nflows, n, nslot))
    nrow = max(slots) + 2
    want = np.full((nrow, 4), 777.0)
    for k, (off, ln) in enumerate(cores):
        off, ln = _clamp(off, ln, length)
        e0, e1 = off // 2, (off + ln) // 2
        core = planes[:, k, e0:e1].astype(np.float64)
        planes[:, k, :e0] = np.nan
        planes[:, k, e1:] = np.nan
        if slots[k] >= 0:
            want[slots[k]] = [np.square(core).sum(), acc[:, k, :nslot - 1].sum(),
                              sum(acc[f, k, nslot - 1] / (2 << (f // n_flow)) for f in range(nflows)), ln]
    pd = dev(np.concatenate([np.full(offset, np.nan, dtype=np.float32), planes.reshape(-1)]))
    part = torch.full((nrow, 4), 777.0, dtype=torch.float64, device="cuda")
    off_d, len_d, slot_d, accd = _i32(o for o, _ in cores), _i32(ln for _, ln in cores), _i32(slots), dev(acc)
    outs = []
    for _ in range(2):
        rc = lib.fwn_window_sums(pd.data_ptr() + 4 * offset, n, length, off_d.data_ptr(), len_d.data_ptr(), accd.data_ptr(), nflows, n_flow,
                                 slot_d.data_ptr(), part.data_ptr(), None)
        assert rc == 0, lib.fwn_last_error()
        outs.append(part.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])
    got = outs[0]
    assert np.isfinite(got).all(), (length, cores)
    assert np.array_equal(got[:, 3], want[:, 3])
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=1e-12, atol=1e-12)


def test_window_sums_kernel_alone():
    lib = _lib.load()
    # L / 2 = 37 elements per plane: the rows of the planes sit on every 4-byte phase.  From 0, a middle range, up to the
    # end, one element per plane, everything, nothing, clamped tables, a negative slot (writes nothing)
    cores = [(0, 20), (22, 30), (60, 14), (0, 2), (34, 2), (72, 2), (0, 74), (10, 0), (-4, 12), (70, 100)]
    slots = [3, 0, 9, 1, -1, 4, 11, 6, 2, 7]
    for offset in (0, 1, 2, 3):
        _sums_case(lib, 74, cores, slots, nflows=4, n_flow=2, offset=offset)
    _sums_case(lib, 2 * 70001, [(2, 140000), (0, 140002), (70000, 6)], [2, 1, 0], nflows=6, n_flow=3)          # longer than one sweep of the lanes
    _sums_case(lib, 64, [(16, 32)], [0], nflows=1, n_flow=1)


# ---- 2. the latent scatter ------------------------------------------------------------------------------------------------
def _time_order_ref(planes, n_block, n_flow):
    """planes [2][n][L / 2] -> [n][L]: un-squeezes of ``z_planes_to_squeezed``."""
    sq = z_planes_to_squeezed(torch.from_numpy(planes), n_block, n_flow).numpy()
    return R.time_order(sq, n_block)


def _latent_case(lib, n_block, n_flow, length, cores, out_offs, total, base=0, zbuf=None):
    n = len(cores)
    rng = np.random.default_rng(length + n_block * 31 + n_flow)
    planes = rng.standard_normal((2, n, length // 2)).astype(np.float32)
    ref = _time_order_ref(planes, n_block, n_flow)
    sentinel = np.float32(-12345.5)
    z = torch.full((total,), float(sentinel), dtype=torch.float32, device="cuda") if zbuf is None else zbuf
    want = np.full(total, sentinel, dtype=np.float32)
    for k, ((off, ln), o) in enumerate(zip(cores, out_offs)):
        off, ln = _clamp(off, ln, length)
        want[o - base:o - base + ln] = ref[k, off:off + ln]
    pd = dev(planes)
    off_d, len_d, out_d = _i32(o for o, _ in cores), _i32(ln for _, ln in cores), _i64(out_offs)     # held until the launch has run
    rc = lib.fwn_window_scatter_latent(pd.data_ptr(), n, length, (n_block * n_flow) & 1, off_d.data_ptr(), len_d.data_ptr(),
                                       out_d.data_ptr(), z.data_ptr(), None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    got = z[base:base + total].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n_block, n_flow, length, cores, out_offs)


@pytest.mark.parametrize("n_block,n_flow", [(2, 2), (2, 3), (5, 2), (5, 1), (5, 3)])
def test_latent_scatter_is_the_unsqueezed_latent_bit_for_bit(n_block, n_flow):
    lib = _lib.load()
    length = 9 * (1 << n_block) * 2
    unit = 1 << n_block
    # cores on the unit (what a plan gives), sentinels between them: from 0, a middle one, up to the end, one unit, all, none
    cores = [(0, 3 * unit), (4 * unit, 5 * unit), (length - 2 * unit, 2 * unit), (7 * unit, unit), (0, length), (unit, 0)]
    outs, at = [], 5
    for _, ln in cores:
        outs.append(at)
        at += ln + 3                                                           # odd gaps: destinations on every phase of 8 bytes
    _latent_case(lib, n_block, n_flow, length, cores, outs, at + 8)
    outs = [2 * (o // 2) for o in outs]                                        # and 8-byte aligned destinations
    _latent_case(lib, n_block, n_flow, length, cores, outs, at + 8)
    # off the unit too - odd starts and lengths, clamped tables: the kernel is stated per sample
    cores = [(1, 7), (3, 2 * unit + 1), (length - 5, 5), (-2, 4), (length - 3, 100), (6, 1)]
    outs, at = [], 4
    for off, ln in cores:
        outs.append(at)
        at += _clamp(off, ln, length)[1] + 2
    _latent_case(lib, n_block, n_flow, length, cores, outs, at + 8)


def test_latent_scatter_past_2_31_elements():
    lib = _lib.load()
    n_block, n_flow, length = 5, 2, 64 * 32
    far = (1 << 31) + 40
    zbuf = torch.empty(far + length + 4096, dtype=torch.float32, device="cuda")
    zbuf[:4096] = -12345.5                                                     # where a 32-bit byte offset would land
    zbuf[far - 1024:] = -12345.5
    cores, outs = [(32, length - 64), (0, 96)], [far + 7, far - 500]
    _latent_case(lib, n_block, n_flow, length, cores, outs, 1024 + length + 4096, base=far - 1024, zbuf=zbuf)
    assert bool((zbuf[:4096] == -12345.5).all())


# ---- 3. forward_windowed against the oracle's whole-clip forward ---------------------------------------------------------------
_MODELS, _STOCK = {}, {}


def _model(cfg, units):
    key = repr(cfg)
    if key not in _MODELS:
        case = R.oracle_case(cfg, units)
        _MODELS[key] = FloWaveNet(case["hp"]).load_params(case["params"])
    return _MODELS[key]


def _stock(cfg, units):
    """The same clip at the stock weights, where the scalars are held: (model, fp64 log_p, logdet of the whole clip)."""
    key = repr(cfg)
    if key not in _STOCK:
        case = R.oracle_case(cfg, units)
        params = W.synthetic_params(case["hp"], 99, actnorm="random")
        lp0, ld0, _ = onp.forward(onp.to_f64(params), case["x"].astype(np.float64), case["c"].astype(np.float64), case["hp"])
        _STOCK[key] = (FloWaveNet(case["hp"]).load_params(params), lp0, ld0)
    return _STOCK[key]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cfg,units", H.GEOMETRIES)
def test_forward_windowed_matches_the_oracle_whole_clip_forward(cfg, units, batch):
    """The clip, the plan and the loud weights of the fp64 proof (tests/test_windowed_forward_host.py), as two clips of one call
    (the second a copy: its windows sit at other rows, slots and offsets and share groups with the first's).  z in time order
    against the oracle's whole-clip forward at ``ABS_Z max(1, |z|max)``; the same call with ``halo=0`` must miss that bound.
    The scalars at the stock weights against the oracle's whole-clip scalars.  The one-call ``forward`` of the same clip is
    printed beside each figure.  Measured on an MI355X, z err / bound per geometry: 0.018 / 0.161, 0.147 / 0.327, 0.458 / 0.486,
    0.012 / 0.068, 0.039 / 0.120 (batch 3: the same in the first three, 0.011 and 0.033 in the last two); the one-call
    ``forward`` has 0.018, 0.147, 0.458, 0.012, 0.032 - the bound is about the pass, not the windows, and the one-call pass meets
    it everywhere, so the oracle is the reference at every geometry; halo 0: 5.9, 9.3, 16.5, 1.05, 1.30.  log_p within 1e-4
    relative, logdet within 1.4e-4 of the oracle everywhere."""
    case = R.oracle_case(cfg, units)
    hp, t, window = case["hp"], case["t"], case["window"]
    model = _model(cfg, units)
    x2, c2 = dev(np.repeat(case["x"], 2, axis=0)), dev(np.repeat(case["c"], 2, axis=0))
    lp, ld, z = model.forward_windowed(x2, c2, window, batch=batch, return_z=True)
    assert lp.shape == ld.shape == (2,) and lp.dtype == ld.dtype == torch.float32 and z.shape == (2, t, 1) and z.dtype == torch.float32
    assert torch.isfinite(lp).all() and torch.isfinite(ld).all() and torch.isfinite(z).all()
    z0 = case["z"]
    bound = ABS_Z * max(1.0, float(np.abs(z0).max()))
    zh = z.cpu().numpy()[:, :, 0]
    err = float(np.abs(zh - z0[None]).max())
    _, _, zp1 = model.forward(x2[:1], c2[:1], return_z=True)
    one = R.time_order(z_planes_to_squeezed(zp1, hp.n_block, hp.n_flow).cpu().numpy(), hp.n_block)[0]
    err_one = float(np.abs(one - z0).max())
    cut = model.forward_windowed(x2, c2, window, batch=batch, return_z=True, halo=0)[2].cpu().numpy()[:, :, 0]
    err_cut = float(np.abs(cut - z0[None]).max())
    print("%r batch %d: z err windowed %.3e, one call %.3e, halo 0 %.3e (bound %.3e)" % (cfg, batch, err, err_one, err_cut, bound))
    assert err <= bound, (cfg, batch, err, bound)
    assert err_cut > bound, (cfg, batch, err_cut, bound)            # the control: a seam is seen
    # the scalars, at the stock weights
    stock, lp0, ld0 = _stock(cfg, units)
    lps, lds = stock.forward_windowed(x2, c2, window, batch=batch)
    lp1, ld1 = stock.forward(x2[:1], c2[:1])
    print("one call: log_p %.6f logdet %.6f" % (float(lp1), float(ld1)))
    for k in range(2):
        check_scalars(lps[k], lds[k], lp0, ld0)
    # without return_z: the same scalars, bit for bit
    lp_b, ld_b = model.forward_windowed(x2, c2, window, batch=batch)
    assert torch.equal(lp_b, lp) and torch.equal(ld_b, ld)


# ---- 4. round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,units", H.GEOMETRIES)
def test_round_trip_through_reverse_windowed(cfg, units):
    """At the stock weights, where tests/test_ragged_forward.py holds its round trip."""
    case = R.oracle_case(cfg, units)
    stock, _, _ = _stock(cfg, units)
    xd, cd = dev(case["x"]), dev(case["c"])
    z = stock.forward_windowed(xd, cd, case["window"], return_z=True)[2]
    back = stock.reverse_windowed(z, cd, case["window"]).cpu().numpy()
    bound = ABS_WAV * max(1.0, float(np.abs(case["x"]).max()))
    err = float(np.abs(back - case["x"]).max())
    print("%r: round trip max err %.3e, bound %.3e" % (cfg, err, bound))
    assert err <= bound, (cfg, err, bound)


# ---- 5. the full model ----------------------------------------------------------------------------------------------------
def test_full_model_windowed_matches_the_golden_10s_clip():
    """BASELINE configs[3] (one 10 s clip, T = 220 672) at window 65 536 - 4 windows - against the committed fp64 ``log_p``,
    ``logdet`` and ``z``, ActNorm initialised by the golden's own forward: the case and the bounds of
    test_baseline_configs_at_their_real_sizes_match_golden (tests/test_gpu_parity.py), the half-ulp allowance for the fp16 z
    included."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    name = "full_b8f6_T220672_10s"
    over, b, t, actnorm, ddi = mg.CASES[name]
    hp = mg.hp_of(over)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    half_ulp = 2.0 ** -11 if g["z"].dtype == np.float16 else 0.0
    model = FloWaveNet(hp, init=True).load_params(W.synthetic_params(hp, 1234, actnorm=actnorm))
    inp = W.synthetic_inputs(hp, b, t)
    x, c = dev(inp["x"]), dev(inp["c"])
    with pytest.raises(ValueError, match="init"):
        model.forward_windowed(x, c, 65536)
    model.forward(x, c)                                             # the data-dependent ActNorm init
    assert len(WIN.plan_windows(t, 65536, hp)) == 4 and WIN.halo_samples(hp) == 15872
    lp, ld, z = model.forward_windowed(x, c, 65536, return_z=True)
    check_scalars(lp[0], ld[0], float(g["log_p"]), float(g["logdet"]))
    z0 = R.time_order(g["z"].astype(np.float32), hp.n_block)
    zh = z.cpu().numpy()[:, :, 0]
    assert zh.shape == z0.shape == (b, t)
    err = np.maximum(np.abs(zh - z0) - half_ulp * np.abs(z0), 0.0).reshape(-1)
    mean, p9999, worst = float(err.mean()), float(np.quantile(err, 0.9999)), float(err.max())
    print("z error over %d samples: mean %.3e  p99.99 %.3e  max %.3e" % (err.size, mean, p9999, worst))
    assert mean < Z_MEAN and p9999 <= Z_P9999 and worst <= Z_MAX, (mean, p9999, worst)


# ---- 6. past what one call can address ------------------------------------------------------------------------------------
def test_a_clip_past_the_ceiling_is_scored_and_exact_at_its_seams():
    hp = small_hparams()
    unit, h, window = WIN.unit_samples(hp), WIN.halo_samples(hp), 262144
    t = 4194304 + 16 * unit
    params = H.loud_params(hp)
    p64 = onp.to_f64(params)
    model = FloWaveNet(hp).load_params(params)
    gen = torch.Generator().manual_seed(3)
    c = torch.rand(1, t // hp.hop_size, hp.num_mels, generator=gen).cuda()
    x = (0.3 * torch.randn(1, t, 1, generator=gen)).clamp(-0.999, 0.999).cuda()
    with pytest.raises(_lib.FwnError, match="exceeds"):
        model.forward(x, c)
    lp, ld, z = model.forward_windowed(x, c, window, return_z=True)
    assert z.shape == (1, t, 1) and torch.isfinite(z).all()
    seam = round(t / 2 / window) * window
    for a in (0, seam - 2 * unit, t - 4 * unit):                    # clip start, across the seam nearest the middle, clip end
        b = a + 4 * unit
        lo, hi = max(0, a - h), min(t, b + h)
        xw = x[0, lo:hi, 0].cpu().numpy().astype(np.float64)
        cw = c[0, lo // hp.hop_size:hi // hp.hop_size].cpu().numpy().astype(np.float64)
        z0 = R.forward_terms(p64, xw[None, :, None], cw[None], hp)[0][a - lo:b - lo]
        got = z[0, a:b, 0].cpu().numpy()
        bound = ABS_Z * max(1.0, float(np.abs(z0).max()))
        err = float(np.abs(got - z0).max())
        print("span [%d, %d): err %.3e (bound %.3e)" % (a, b, err, bound))
        assert err <= bound, (a, err, bound)
        assert float(np.abs(got).max()) > 0.0
    lp_z = 0.5 * (-np.log(2.0 * np.pi) - float(z.double().square().sum()) / t)
    print("log_p %.9f, from the returned z in fp64 %.9f" % (float(lp[0]), lp_z))
    assert abs(float(lp[0]) - lp_z) <= 1e-6 * abs(lp_z)
    ld_other = model.forward_windowed(x, c, 1048576)[1]            # another plan, other groups
    print("logdet %.6f at window %d, %.6f at window 1048576" % (float(ld[0]), window, float(ld_other[0])))
    assert abs(float(ld[0]) - float(ld_other[0])) <= ABS_LOGDET * max(1.0, abs(float(ld_other[0])))


# ---- 7. determinism, and the stream ---------------------------------------------------------------------------------------------
def test_two_identical_calls_and_the_stream_give_identical_bits():
    case = R.oracle_case(*H.GEOMETRIES[0])
    hp = case["hp"]
    model = _model(*H.GEOMETRIES[0])
    h, hop, window = WIN.halo_samples(hp), hp.hop_size, 256
    frames = 150
    gen = torch.Generator().manual_seed(5)
    c = torch.rand(1, frames, hp.num_mels, generator=gen).cuda()
    x = (0.3 * torch.randn(1, frames * hop, 1, generator=gen)).cuda()
    for batch in (1, 3):
        a = model.forward_windowed(x, c, window, batch=batch, return_z=True)
        b = model.forward_windowed(x, c, window, batch=batch, return_z=True)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), batch
    want = model.forward_windowed(x, c, window, batch=1, return_z=True)
    first = (window + h) // hop                                     # the frame whose arrival completes the first window
    for size in (1, 7, 64):
        st = model.forward_stream(window=window)
        parts, arrived, first_at = [], 0, None
        while arrived < frames:
            f = min(size, frames - arrived)
            xs, cs = x[0, arrived * hop:(arrived + f) * hop, 0], c[0, arrived:arrived + f]
            part = st.push(xs, cs) if size != 7 else st.push(xs.cpu().numpy(), cs.cpu().numpy())
            assert part.dtype == torch.float32 and part.dim() == 1
            arrived += f
            if part.numel() and first_at is None:
                first_at = arrived
            assert st.retained_frames <= (window + 2 * h) // hop + size
            parts.append(part)
        assert first_at is not None and first_at - size < first <= first_at, (size, first_at, first)
        rest, lp, ld = st.finish()
        parts.append(rest)
        assert torch.equal(torch.cat(parts), want[2][0, :, 0]), size
        assert torch.equal(lp, want[0][0]) and torch.equal(ld, want[1][0]), size
    st = model.forward_stream(window=window, return_z=False)
    assert st.push(x[0, :, 0], c[0]).numel() == 0
    rest, lp, ld = st.finish()
    assert rest.numel() == 0 and torch.equal(lp, want[0][0]) and torch.equal(ld, want[1][0])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    hp = small_hparams()
    params = W.synthetic_params(hp, 99, actnorm="random")
    model = FloWaveNet(hp).load_params(params)
    inp = W.synthetic_inputs(hp, 2, 256, want=("x", "c"))
    x, c = dev(inp["x"]), dev(inp["c"])
    with pytest.raises(ValueError, match="init"):
        FloWaveNet(hp, init=True).load_params(params).forward_windowed(x, c, 64)
    fp8 = FloWaveNet(hp, gate_fp8=True).load_params(params)
    with pytest.raises(ValueError, match="gate_fp8"):
        fp8.forward_windowed(x, c, 64)
    with pytest.raises(ValueError, match="gate_fp8"):
        fp8.forward_stream(window=64)
    with pytest.raises(ValueError):
        model.forward_windowed(x, c, 24)                            # no multiple of the unit
    with pytest.raises(ValueError):
        model.forward_windowed(x[:, :250], c, 64)
    # the C entry by itself
    lib = _lib.load()
    n, length = 2, 64
    desc = C.byref(model._packed.model_desc)
    nbytes = lib.fwn_forward_windows_workspace_bytes(desc, n, length)
    assert nbytes > lib.fwn_ragged_forward_workspace_bytes(desc, n, length) > 0
    assert lib.fwn_forward_windows_workspace_bytes(desc, 32768, 16) == 0
    assert lib.fwn_forward_windows_workspace_bytes(C.byref(fp8._packed.model_desc), n, length) == 0
    assert lib.fwn_forward_windows_workspace_bytes(desc, n, length + 1) == 0
    ws = torch.empty(nbytes + 512, dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
    x32, c32 = x.float().contiguous(), c.float().contiguous()
    t64 = torch.zeros(16, dtype=torch.int64, device="cuda")          # rows 0, 0; z offsets 0, 0 - overwritten below
    t64[8], t64[9] = 0, 64
    t32 = torch.tensor([0, 0, 64, 64, 0, 1, 0, 0], dtype=torch.int32).cuda()        # core_off | core_len | slot
    acc = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    zf = torch.zeros(128, dtype=torch.float32, device="cuda")
    good = dict(m=desc, n=n, L=length, x=x32.data_ptr(), xrow=t64.data_ptr(), mel=c32.data_ptr(), melrow=t64.data_ptr(),
                off=t32.data_ptr(), len=t32.data_ptr() + 8, slot=t32.data_ptr() + 16, acc=acc.data_ptr(), zoff=t64.data_ptr() + 64,
                z=zf.data_ptr(), ws=wsp, wsn=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fwn_model_forward_windows(a["m"], a["n"], a["L"], a["x"], a["xrow"], a["mel"], a["melrow"], a["off"], a["len"], a["slot"],
                                             a["acc"], a["zoff"], a["z"], a["ws"], a["wsn"], None)

    assert call() == 0, lib.fwn_last_error()
    assert call(z=None, zoff=None) == 0, lib.fwn_last_error()       # no latent wanted: no offsets needed
    torch.cuda.synchronize()
    assert float(acc[0, 3]) == 64.0 and float(acc[1, 3]) == 64.0
    for name in ("x", "xrow", "mel", "melrow", "off", "len", "slot", "acc", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.fwn_last_error(), (name, lib.fwn_last_error())
    assert call(zoff=None) == -1 and b"null" in lib.fwn_last_error()
    for name, by in (("xrow", 4), ("melrow", 4), ("zoff", 4), ("acc", 4), ("off", 2), ("len", 2), ("slot", 2), ("x", 2), ("mel", 2), ("z", 2)):
        assert call(**{name: good[name] + by}) == -1 and b"aligned" in lib.fwn_last_error(), (name, lib.fwn_last_error())
    assert call(ws=wsp + 128) == -1 and b"256" in lib.fwn_last_error()
    assert call(n=32768, L=16) == -1 and b"32767" in lib.fwn_last_error()
    assert call(m=C.byref(fp8._packed.model_desc)) == -1 and b"fp8" in lib.fwn_last_error()
    assert call(wsn=nbytes - 256) == -3 and b"workspace" in lib.fwn_last_error()
    # the kernels' own entries
    for fn, args in ((lib.fwn_window_logdet_rows, (None, 1, 4, 1, zf.data_ptr(), None, t32.data_ptr(), t32.data_ptr(), 2, acc.data_ptr(), None)),
                     (lib.fwn_window_logdet_rows, (zf.data_ptr(), 1, 4, 3, zf.data_ptr(), None, t32.data_ptr(), t32.data_ptr(), 6, acc.data_ptr(), None)),
                     (lib.fwn_window_sums, (zf.data_ptr(), 1, 63, t32.data_ptr(), t32.data_ptr(), acc.data_ptr(), 1, 1, t32.data_ptr(), acc.data_ptr(), None)),
                     (lib.fwn_window_scatter_latent, (zf.data_ptr(), 1, 64, 0, t32.data_ptr(), t32.data_ptr(), t64.data_ptr() + 4, zf.data_ptr(), None)),
                     (lib.fwn_forward_windows_finish, (acc.data_ptr(), t32.data_ptr(), None, 1, zf.data_ptr(), None))):
        assert fn(*args) == -1, fn
    torch.cuda.synchronize()


# ---- 9. score --window ------------------------------------------------------------------------------------------------------
def test_score_cli_window(tmp_path):
    """A long clip's record is ``forward_windowed``'s; the short clips' records are those of a run without the flag, bit for
    bit (one of them shares its call with the long clip in both runs)."""
    from tf_flowavenet_amd import score as SC
    hp = small_hparams()
    params = W.synthetic_params(hp, 2, actnorm="random")
    for sub in ("ckpt", "audios", "mels"):
        (tmp_path / sub).mkdir()
    np.savez(tmp_path / "ckpt" / "flowavenet_model.npz", **params)
    rng = np.random.default_rng(0)
    clips = (("a1.npy", "m1.npy", 5), ("a2.npy", "m2.npy", 130), ("a3.npy", "m3.npy", 7), ("a4.npy", "m4.npy", 100))
    data, lines = {}, []
    for audio, mel, frames in clips:
        a = np.clip(0.3 * rng.standard_normal(frames * hp.hop_size), -0.999, 0.999).astype(np.float32)
        m = rng.random((frames, hp.num_mels), dtype=np.float32)
        np.save(tmp_path / "audios" / audio, a)
        np.save(tmp_path / "mels" / mel, m)
        lines.append("%s|%s|%d|0|text" % (audio, mel, len(a)))
        data[audio] = (a, m)
    (tmp_path / "train.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    base = dict(saved_dir=str(tmp_path / "ckpt"), base_dir=str(tmp_path), batch=8, max_pad_frac=0.3)
    plain = SC.score(type("A", (), dict(out=str(tmp_path / "plain.jsonl"), **base))(), hp)
    window = 1700                                                   # rounded up to 1712: a2 (2080 samples) is long, a4 (1600) is not
    recs = SC.score(type("A", (), dict(out=str(tmp_path / "win.jsonl"), window=window, **base))(), hp)
    assert [json.loads(line) for line in (tmp_path / "win.jsonl").read_text(encoding="utf-8").splitlines()] == recs
    assert [r["name"] for r in recs] == [r["name"] for r in plain] == [a for a, _, _ in clips]
    model = FloWaveNet(hp).load_params(params)
    a, m = data["a2.npy"]
    lp, ld = model.forward_windowed(dev(a[None, :, None]), dev(m[None]), window=1712, batch=8)
    p64 = onp.to_f64(params)
    for r, r0 in zip(recs, plain):
        if r["name"] == "a2.npy":
            assert r["samples"] == 2080 and r["log_p"] == float(lp[0]) and r["logdet"] == float(ld[0]) and r["nll"] == -(r["log_p"] + r["logdet"])
            check_scalars(r["log_p"], r["logdet"], *onp.forward(p64, a.astype(np.float64)[None, :, None], m.astype(np.float64)[None], hp)[:2])
        else:
            assert r == r0, (r, r0)
