"""Three inference stages through the C ABI against the plain NumPy fp64 references of tests/test_infer_stage_refs.py
(proved there on the CPU): fwn_res in its four tile forms, fwn_front in every form the entry point reaches, and the
ActNorm + coupling + log-det epilogue of the tail in every (form, ZeroConv pair-tile count, direction).  The single-flow
oracle tests hold these stages only behind a ZeroConv of N(0, 0.02^2) kernels and a 2e-2 absolute bound; here each
kernel is alone, on operands of the test's own, with two kinds of case as in tests/test_train_gemms.py:

(a) exact: small integers (and power-of-two scales), every partial sum an integer below 2^24 and so exact in fp32 in any
    order: the kernel must give the reference's bits - a wrong tap at a clip edge, a dropped residual add in one column
    group, a wrong chunk or tile edge shows whatever its size.
(b) bounded: random normal operands against per-element bounds, none fitted (u = 2^-24, the factor 2 is head-room):
    fwn_res:   2 (256 + 4) u terms + 2 u |want| + 2^-8 |want|      (K = 256 products, the epilogue, the bf16 cast)
    fwn_front: 2 (3 Ch + 4) u terms + 2 u |want| + 2^-8 |want|     (fp32 VALU form)
               the same + 2^-16 terms                               (MFMA forms: x enters as hi + lo bf16, 16 mantissa bits,
                                                                     a relative 2^-17)
    terms = sum |x w| + |bias| (+ |h|), with x the ActNorm-applied plane.
    tail epilogue: planes within 1e-5 max(1, |want|max), sum(partial) within 1e-4 max(1, sum |a_l3| + |b_l3| + |ls|), the round
    trip within 2e-5 max(1, |x|max): the figures tests/test_train.py uses for the same expressions with __expf.

Every case asserts the form it is there to reach through the rules restated in test_infer_stage_refs.py.  Outputs start
as a sentinel or NaN, every buffer is followed by a guard that must come back untouched, inputs must come back unchanged.
Not reachable through the entry points, and so not here: launch_ring's 256 x 128 arm for N = 256 (fwn_launch_res takes
the depth-2 128 x 128 tile at the same row count) and the xprep_kernel + ring form of the front conv (it needs a plane
that is not 16-byte aligned, which fwn_front refuses: the ALIGNED16 REQUIRE in csrc/api.hip).  fwn_res never runs in
place: both sequencers alternate two h buffers (csrc/api.hip flow_run_impl, sg.h[l]), so aliasing is not tested.

Worst err / bound measured on an MI355X (the last test prints the table of the session):
    res    split-K 64 x 64 0.985, 64 x 128 0.984, 128 x 128 depth 3 0.985, depth 2 0.985
    front  VALU 16-row and 64-row forms 0.990 - 0.996 (Ch 1 .. 16); MFMA Ch 16 / 32 / 64 / 128 0.985 / 0.980 / 0.961 / 0.927;
           gemm128<1> 0.965 - 0.978, gemm128<2> 0.986
    tail   every (form, pair tiles): planes 0.006 - 0.027, round trip 0.007 - 0.014, log-det sum below 0.001
The res and front ratios sit just under 1 by construction: the bound's leading term 2^-8 |want| IS the worst case of one bf16
rounding (half an ulp of a value at the bottom of its binade), and among 10^5 - 10^7 outputs some land there; what is left
over is the accumulation term, which the wider K of the MFMA forms makes larger.  A mutation of sqrt(1/2) by 1e-4 relative
fails the bounded res cases for that reason."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import _lib, packing
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd.model import FloWaveNet

from test_train_stages import GUARD, SENT, U, assert_within, dev, guard_intact, host, scratch, stream
from test_train_gemms import bdev, bits32, to_bf16
from test_infer_stage_refs import (SQRT_HALF_F32, TAIL_CASES, ez_planes, front_form, npt_of, ref_front, ref_res,
                                   ref_tail_epilogue, res_form, res_row_counts, tail_form, tail_partials_bound, tail_slots)
from test_train_gemm_refs import ref_gemm

pytestmark = pytest.mark.gpu

BIG = 1e30
RATIOS = {}          # worst err / bound per (stage, form) over the bounded cases (printed by the last test)


def note_ratio(key, got, want, bound, what):
    assert_within(got, want, bound, "%s: %s" % (key, what))
    err = np.abs(got.astype(np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    nz = bound > 0
    r = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return r


def build_full():
    """The full-size model on the synthetic parameters, ActNorm initialised from data (the fixture of test_gpu_parity.py)."""
    hp = default_hparams()
    params = W.synthetic_params(hp, 1234)
    model = FloWaveNet(hp, init=True).load_params(params)
    inp = W.synthetic_inputs(hp, 8, 16128, want=("x", "c"))
    model.forward(torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["c"]).cuda())
    torch.cuda.synchronize()
    return hp, model, params


@pytest.fixture(scope="module")
def full():
    return build_full()


def p64_of(params, prefix):
    return {k: np.asarray(v, np.float64) for k, v in params.items() if k.startswith(prefix)}


def dev_read(pm, ptr, n, dtype):
    """n elements of `dtype` at device address ptr, which lies inside one of the packed model's own tensors."""
    size = torch.empty(0, dtype=dtype).element_size()
    for t in pm.tensors:
        b0, nb = t.data_ptr(), t.numel() * t.element_size()
        if b0 <= ptr and ptr + n * size <= b0 + nb:
            raw = t.reshape(-1).view(torch.uint8)[ptr - b0: ptr - b0 + n * size]
            return raw.clone().view(dtype)
    raise AssertionError("address %#x is not inside a packed tensor" % ptr)


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def fold_ok(packed, fold):
    """bf16(fp32(fold)): one bf16 rounding of an fp32 value within 4 u of the fp64 fold.  Round to nearest moves a value by at
    most half an ulp of its binade, 2^(e - 8) for |w| in [2^e, 2^(e + 1)): that is 2^-9 |w| only at the top of the binade and
    2^-8 |w| at its bottom (bf16 keeps 8 significant bits), so a flat 2^-9 |w| - the first form of this check - fails on
    correctly rounded values (0.0390625 for 0.03894084: half an ulp, 2^-8.3 relative).  The half ulp itself is asserted."""
    half_ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(fold), 1e-300))) - 8)
    return np.abs(packed - fold) <= half_ulp + 4.0 * U * np.abs(fold)


def flow_copy(model, hp, blk, flow=0):
    return _lib.FlowDesc.from_buffer_copy(model._packed.flow_descs[blk * hp.n_flow + flow])


def same_bits_f32(got, want):
    """Bit equality of two fp32 arrays, +0 and -0 alike (fmaxf(-0, +0) may return either)."""
    return bits32(np.asarray(got, np.float32) + np.float32(0.0)) == bits32(np.asarray(want, np.float32) + np.float32(0.0))


# =================================================================== fwn_res
def test_packed_res_operands_equal_the_fp64_fold(full):
    """What ties the [256][256] / [256] layout of the cases below to the product: the model's own Wres / bres are the
    weight-norm fold of the parameters, W[n][k] = v[k][n] g[n] / ||v[:, n]||, rounded once to bf16."""
    hp, model, params = full
    for blk, flow in ((0, 0), (3, 1), (7, 5)):
        d = model._packed.flow_descs[blk * hp.n_flow + flow]
        rp = W.flow_prefix(blk, flow) + "/WaveNet/ResBlock_0"
        p = p64_of(params, rp + "/res_conv")
        fold = onp.wn_kernel_1d(p, rp + "/res_conv")[0].T
        Wr = f64(dev_read(model._packed, d.Wres[0], 256 * 256, torch.bfloat16)).reshape(256, 256)
        assert fold_ok(Wr, fold).all() and np.abs(fold).max() > 0.01
        b = f64(dev_read(model._packed, d.bres[0], 256, torch.float32))
        assert (np.abs(b - p[rp + "/res_conv/bias"]) <= 4.0 * U * np.abs(b)).all()


RES_ROWS = res_row_counts()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("form,M", [(f, m) for f, ms in RES_ROWS.items() for m in ms])
def test_res_every_form(full, form, M, exact):
    """fwn_res = (h + o Wres^T + b) sqrt(1/2) on a descriptor copy whose Wres[0] / bres[0] are the test's own: the split-K
    64 x 64 tile, the 64 x 128 and 128 x 128 ring tiles and the depth-2 128 x 128 tile, each at its first row count (a
    one-row last tile) and at an exact multiple (row counts derived in test_infer_stage_refs.py).
    exact: h + acc + b is an integer s below 2^24, the result bf16(fp32(s) fp32(0.70710678118654752)) bit for bit.
    bounded: h dominates the sum (|h| ~ 3, |o W| ~ 0.3) so that the bound is about the bf16 cast of the product alone."""
    hp, model, _ = full
    lib = _lib.load()
    assert res_form(M) == form
    rng = np.random.default_rng(2 * M + exact)
    if exact:
        o = rng.integers(-3, 4, (M, 256)).astype(np.float32)
        Wr = rng.choice([-1.0, 0.0, 1.0], (256, 256), p=[0.25, 0.5, 0.25]).astype(np.float32)
        h = rng.integers(-8, 9, (M, 256)).astype(np.float32)
        b = rng.integers(-4, 5, 256).astype(np.float32)
    else:
        o = to_bf16(rng.standard_normal((M, 256)) * 0.5)
        Wr = to_bf16(rng.standard_normal((256, 256)) * 0.03)
        h = to_bf16(rng.standard_normal((M, 256)) * 3.0)
        b = (rng.standard_normal(256) * 0.1).astype(np.float32)
    d = flow_copy(model, hp, 0)
    d_o, d_h, d_W, d_b = bdev(o), bdev(h), bdev(Wr), dev(b)
    d.Wres[0], d.bres[0] = d_W.data_ptr(), d_b.data_ptr()
    o0, h0 = d_o.clone(), d_h.clone()
    d_out = torch.full((M * 256 + GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fwn_res(C.byref(d), 0, d_o.data_ptr(), d_h.data_ptr(), d_out.data_ptr(), M, stream()), "fwn_res")
    torch.cuda.synchronize()
    assert all(guard_intact(t, n) for t, n in ((d_out, M * 256), (d_o, M * 256), (d_h, M * 256), (d_W, 65536), (d_b, 256)))
    assert torch.equal(d_o.view(torch.int16), o0.view(torch.int16)) and torch.equal(d_h.view(torch.int16), h0.view(torch.int16))
    got = d_out[:M * 256].float().cpu().numpy().reshape(M, 256)
    if exact:
        s = ref_gemm([(o, 256, 0, 0)], Wr, M, 256, bias=b, R=h, with_abs=False)[0]
        assert np.abs(s).max() < 2.0 ** 24 and (s == np.round(s)).all()
        want = to_bf16(s.astype(np.float32) * SQRT_HALF_F32)
        bad = ~same_bits_f32(got, want)
        assert not bad.any(), "res %s M %d: %d of %d elements differ from the exact result, first at %s" % (
            form, M, int(bad.sum()), bad.size, np.unravel_index(np.argmax(bad), bad.shape))
    else:
        want, terms = ref_res(o, h, Wr, b)
        bound = 2.0 * (256 + 4) * U * terms + 2.0 * U * np.abs(want) + 2.0 ** -8 * np.abs(want)
        r = note_ratio("res %s" % form, got, want, bound, "M %d" % M)
        print("res %-12s M %5d  err / bound %.3f" % (form, M, r))


# =================================================================== fwn_front
def front2_layout(Wl, Ch):
    """Logical [256][3][Ch] -> Wfront2 as include/fwn.h lays it out: K = tap 2 Cp + (hi | lo) Cp + tau with Cp = Ch (Ch >= 32)
    or 32 (Ch = 16: the channels tau >= 16 of both halves zero)."""
    cp = max(Ch, 32)
    out = np.zeros((256, 3, 2, cp), np.float32)
    out[:, :, 0, :Ch] = Wl
    out[:, :, 1, :Ch] = Wl
    return out.reshape(256, 6 * cp)


def test_packed_front_operands_equal_the_fp64_fold(full):
    """The model's own Wfront ([256][kfpad], K = tap Ch + tau, finite padding), Wfront2 (the hi | lo layout of fwn.h, Ch = 16
    padded to 32 channels per half with zeros) and bfront against the weight-norm fold of the parameters read through
    packing.front_src_k (proved against the oracle's conv in test_infer_stage_refs.py); Wfront2 holds Wfront's bits."""
    hp, model, params = full
    for blk in range(hp.n_block):
        ch, flow = 1 << blk, blk % hp.n_flow
        d = model._packed.flow_descs[blk * hp.n_flow + flow]
        fp = W.flow_prefix(blk, flow) + "/WaveNet/Conv_front"
        p = p64_of(params, fp)
        fold = onp.wn_kernel_1d(p, fp).reshape(3 * ch, 256)[packing.front_src_k(blk)[:3 * ch]].T       # [256][tap Ch + tau]
        assert d.kfpad == packing.roundup(3 * ch, 64)
        Wf = f64(dev_read(model._packed, d.Wfront, 256 * d.kfpad, torch.bfloat16)).reshape(256, d.kfpad)
        assert fold_ok(Wf[:, :3 * ch], fold).all() and np.isfinite(Wf[:, 3 * ch:]).all()
        b = f64(dev_read(model._packed, d.bfront, 256, torch.float32))
        assert (np.abs(b - p[fp + "/bias"]) <= 4.0 * U * np.abs(b)).all()
        if ch >= 16:
            cp = max(ch, 32)
            W2 = f64(dev_read(model._packed, d.Wfront2, 256 * 6 * cp, torch.bfloat16)).reshape(256, 6 * cp)
            assert np.array_equal(W2, front2_layout(Wf[:, :3 * ch].reshape(256, 3, ch), ch).astype(np.float64))
        else:
            assert not d.Wfront2


def front_geometries(H, big):
    """(M, Ti) with M % Ti == 0 for a form of tile height H: Ti = 1 (only the centre tap survives), 2, H (every tile boundary
    a clip edge), H - 1 and H + 1 (the edge walks through every row position of the tile), one clip; M no multiple of the tile
    except where Ti = H forces it.  big: the smallest such M from `big` rows on, else a few hundred rows."""
    out = []
    for ti in (1, 2, H, H - 1, H + 1, 0):
        if ti == 0:
            m = (big or 300) + 1
            out.append((m, m))
            continue
        n = -(-(big or 300) // ti)
        while ti != H and (n * ti) % H == 0:
            n += 1
        out.append((n * ti, ti))
    return out


def front_operands(model, hp, blk, have_W2, exact, rng):
    """A descriptor copy for the case, and what the reference needs: (d, an_a [4][Ch], W [256][3 Ch], bias, keep-alive list).
    exact: the test's own an (integer shift, scale 1 | 2 | 4), integer weights with six non-zeros per row and an integer bias,
    in the test's own Wfront (1e30 in the padding columns: finite padding is the contract) and Wfront2.
    bounded: the model's own operands, ActNorm initialised from data."""
    ch = 1 << blk
    d = flow_copy(model, hp, blk)
    keep = []
    if exact:
        an = np.zeros((2, 4, ch), np.float32)
        an[:, 0] = rng.integers(-2, 3, (2, ch))
        an[:, 1] = rng.choice([1.0, 2.0, 4.0], (2, ch))
        an[:, 2] = 1.0 / an[:, 1]
        Wl = np.zeros((256, 3 * ch), np.float32)
        for n in range(256):
            k = rng.choice(3 * ch, min(6, 3 * ch), replace=False)
            Wl[n, k] = rng.choice([-1.0, 1.0], k.size)
        bias = rng.integers(-4, 5, 256).astype(np.float32)
        Wf = np.full((256, d.kfpad), to_bf16(np.float32(BIG)), np.float32)
        Wf[:, :3 * ch] = Wl
        d_an, d_W, d_b = dev(an), bdev(Wf), dev(bias)
        d.an, d.Wfront, d.bfront = d_an.data_ptr(), d_W.data_ptr(), d_b.data_ptr()
        keep += [(d_an, an.size), (d_W, Wf.size), (d_b, 256)]
        if have_W2:
            W2 = front2_layout(Wl.reshape(256, 3, ch), ch)
            d_W2 = bdev(W2)
            d.Wfront2 = d_W2.data_ptr()
            keep.append((d_W2, W2.size))
        an_a = an[0]
    else:
        an_a = model._packed.an[(blk, 0)][0].cpu().numpy()
        Wl = f64(dev_read(model._packed, d.Wfront, 256 * d.kfpad, torch.bfloat16)).reshape(256, d.kfpad)[:, :3 * ch]
        bias = f64(dev_read(model._packed, d.bfront, 256, torch.float32))
    if not have_W2:
        d.Wfront2 = None
    return d, an_a, Wl, bias, keep


def run_front(d, xa, M, Ti, apply_an, keep):
    lib = _lib.load()
    d_x = dev(xa)
    d_out = torch.full((M * 256 + GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
    assert d_x.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    _lib.check(lib.fwn_front(C.byref(d), d_x.data_ptr(), d_out.data_ptr(), None, M, Ti, apply_an, stream()), "fwn_front")
    torch.cuda.synchronize()
    assert guard_intact(d_out, M * 256) and guard_intact(d_x, xa.size) and all(guard_intact(t, n) for t, n in keep)
    assert np.array_equal(bits32(host(d_x, xa.shape)), bits32(xa))
    return d_out[:M * 256].float().cpu().numpy().reshape(M, 256)


# (Ch, Wfront2 kept, tile height, rows from which the form starts (0: a few hundred rows), the form)
FRONT_FORMS = (
    [(ch, False, 16, 0, "valu_k%d_r16" % k) for ch, k in ((1, 6), (2, 6), (4, 12), (8, 24), (16, 48))]
    + [(ch, False, 64, 64 * 512, "valu_k%d_r64" % k) for ch, k in ((1, 6), (2, 6), (4, 12), (8, 24), (16, 48))]
    + [(ch, True, 64, 0, "mfma%d" % ch) for ch in (16, 32, 64, 128)]
    + [(ch, False, 64, 0, "gemm128_1") for ch in (32, 64, 128)]
    + [(32, False, 128, 255 * 128 + 1, "gemm128_2")]
)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("Ch,have_W2,H,big,form", FRONT_FORMS, ids=["%s-ch%d" % (f[4], f[0]) for f in FRONT_FORMS])
def test_front_every_form_and_clip_geometry(full, Ch, have_W2, H, big, form, exact):
    """fwn_front = ReLU(conv_k3(ActNorm?(xa)) + b) per clip: front_valu_kernel<R, KMAX> (Ch = 1 .. 8, and 16 through a
    descriptor copy without Wfront2) in its 16-row and 64-row forms, front_mfma_kernel<32, 16 | 32 | 64 | 128>, and
    gemm128_kernel<1 | 2, FrontProb> (Ch >= 32 without Wfront2, which fwn.h allows), over the clip geometries of
    front_geometries and both apply_an values.  exact: integer planes |x| <= 8 (the lo half of the hi | lo pair is 0), so
    ReLU(sum + b) is an integer of at most 6 x 40 + 4 that bf16 holds: bit for bit."""
    hp, model, _ = full
    blk = Ch.bit_length() - 1
    rng = np.random.default_rng(1000 * Ch + 10 * H + exact + (7 if have_W2 else 0) + (big > 0))
    d, an_a, Wl, bias, keep = front_operands(model, hp, blk, have_W2, exact, rng)
    geos = front_geometries(H, big)
    if form == "gemm128_1" and Ch == 32:
        geos.append((255 * 128, 128))                  # the last row count of the 64-row form: one below gemm128_2's first
    mfma = not form.startswith("valu")
    for M, Ti in geos:
        assert M % Ti == 0 and front_form(Ch, have_W2, M) == form, (M, Ti, front_form(Ch, have_W2, M))
        if exact:
            xa = rng.integers(-8, 9, (M, Ch)).astype(np.float32)
        else:
            xa = rng.standard_normal((M, Ch)).astype(np.float32)
        for apply_an in (1, 0):
            got = run_front(d, xa, M, Ti, apply_an, keep)
            want, terms = ref_front(xa, an_a, Wl, bias, Ti, apply_an)
            what = "M %d Ti %d apply_an %d" % (M, Ti, apply_an)
            if exact:
                assert np.abs(want).max() <= 256.0 and (want == np.round(want)).all() and want.max() > 0
                bad = ~same_bits_f32(got, want)
                assert not bad.any(), "front %s Ch %d %s: %d of %d elements differ from the exact result, first at %s" % (
                    form, Ch, what, int(bad.sum()), bad.size, np.unravel_index(np.argmax(bad), bad.shape))
            else:
                bound = 2.0 * (3 * Ch + 4) * U * terms + (2.0 ** -8 + 2.0 * U) * np.abs(want) + (2.0 ** -16 * terms if mfma else 0.0)
                note_ratio("front %s ch%d" % (form, Ch), got, want, bound, what)
    if not exact:
        print("front %-12s Ch %3d  err / bound %.3f" % (form, Ch, RATIOS["front %s ch%d" % (form, Ch)]))


@pytest.mark.parametrize("Ch", [16, 32, 64, 128])
@pytest.mark.parametrize("M,Ti", [(305, 61), (320, 64)])
def test_front_mfma_zero_row_hides_what_lies_outside_a_clip(full, Ch, M, Ti):
    """front_mfma_kernel reads a tap that leaves its clip (or the matrix) from a row of zeros, never from the neighbouring
    row times zero ("0 x NaN is not").  The plane sits one row into a larger buffer; NaN in the row in front of row 0 and in
    every row behind row M - 1 (M = 305: the 15 rows up to the end of the last tile, and more) must change no bit of the
    output.  NaN in the last row of clip 1 and the first row of clip 3 - the row before clip 2's first row and the row after
    its last; with Ti = 64 they are the halo rows of clip 2's tile - poisons those two rows and their neighbour INSIDE their
    own clips (the taps that legitimately read them) and nothing else: every other row keeps its bits, clip 2 whole."""
    hp, model, _ = full
    lib = _lib.load()
    blk = Ch.bit_length() - 1
    d = flow_copy(model, hp, blk)
    assert front_form(Ch, bool(d.Wfront2), M) == "mfma%d" % Ch and M % Ti == 0 and M // Ti == 5
    rng = np.random.default_rng(Ch + M)
    xa = rng.standard_normal((M, Ch)).astype(np.float32)
    tail_rows = 80                                   # guard rows behind the plane: past the end of the last 64-row tile and its halo
    outs = []
    for fill, poison in ((SENT, ()), (float("nan"), ()), (SENT, (2 * Ti - 1, 3 * Ti))):
        buf = torch.full(((1 + M + tail_rows) * Ch,), fill, dtype=torch.float32, device="cuda")
        x = xa.copy()
        for r in poison:
            x[r] = np.nan
        buf[Ch:(1 + M) * Ch] = torch.from_numpy(x.reshape(-1)).cuda()
        d_out = torch.full((M * 256 + GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
        assert (buf.data_ptr() + 4 * Ch) % 16 == 0
        _lib.check(lib.fwn_front(C.byref(d), buf.data_ptr() + 4 * Ch, d_out.data_ptr(), None, M, Ti, 1, stream()), "fwn_front")
        torch.cuda.synchronize()
        assert guard_intact(d_out, M * 256)
        outs.append(d_out[:M * 256].float().cpu().numpy().reshape(M, 256))
    clean, guards_nan, edges_nan = outs
    assert np.isfinite(clean).all() and (clean > 0).any()
    assert np.isfinite(guards_nan).all() and np.array_equal(bits32(guards_nan), bits32(clean))
    hit = np.zeros(M, bool)
    hit[[2 * Ti - 2, 2 * Ti - 1, 3 * Ti, 3 * Ti + 1]] = True
    assert np.isfinite(edges_nan[~hit]).all() and np.array_equal(bits32(edges_nan[~hit]), bits32(clean[~hit]))
    # (finite alone would prove little: fmaxf(NaN, 0) = 0, so a NaN that leaks into a sum leaves a finite 0 - the bits show it)
    assert not np.array_equal(bits32(edges_nan[hit]), bits32(clean[hit]))       # and the rows that do read them saw them


# =================================================================== the tail's epilogue
ZERO_SCALE = {}      # Ch -> the power of two the model's Wzero is multiplied by


def zero_operands(model, hp, d, Ch, zscale, rng):
    """The test's own ZeroConv operands in a descriptor copy: the model's Wzero times a power of two (exact in bf16), and -
    the synthetic parameters leave the ZeroConv bias and scale at 0, so the model's own ezero is all ones - a bias that
    centres log_s at 0.75 and an exp(3 scale) factor between exp(-0.3) and exp(0.3).  Returns (ez, bz [npt 64], keep-alive list)."""
    npt = npt_of(Ch)
    Wz = f64(dev_read(model._packed, d.Wzero, npt * 64 * 256, torch.bfloat16)) * zscale
    ez = np.exp(rng.uniform(-0.3, 0.3, npt * 64)).astype(np.float32)
    bz = (rng.standard_normal(npt * 64) * 0.1).astype(np.float32)
    ls_rows = (np.arange(npt * 64) % 64) < 32
    bz[ls_rows] += (0.75 / ez[ls_rows]).astype(np.float32)
    d_Wz, d_bz, d_ez = bdev(Wz), dev(bz), dev(ez)
    assert np.array_equal(f64(d_Wz[:Wz.size]), Wz)
    d.Wzero, d.bzero, d.ezero = d_Wz.data_ptr(), d_bz.data_ptr(), d_ez.data_ptr()
    return ez, bz, [(d_Wz, Wz.size), (d_bz, bz.size), (d_ez, ez.size)]


def tail_inputs(L, M, Ch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    o = torch.full((L * M * 256 + GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
    o[:L * M * 256] = (torch.rand(L * M * 256, generator=g, device="cuda") * 0.8).to(torch.bfloat16)
    xa = torch.randn(M * Ch, generator=g, device="cuda")
    xb = torch.randn(M * Ch, generator=g, device="cuda")
    return o, xa, xb


def plane_dev(x):
    t = torch.full((x.numel() + GUARD,), SENT, dtype=torch.float32, device="cuda")
    t[:x.numel()] = x
    return t


def tail_forward_train(d, o, xa, xb, M, Ch, nb):
    """fwn_tail_train on fresh copies of the planes -> (planes a, b, partial, S, U, Z) as guarded device tensors."""
    lib = _lib.load()
    pa, pb = plane_dev(xa), plane_dev(xb)
    part = dev(np.zeros(nb, np.float32))
    S, Us = scratch(M * 256, torch.bfloat16), scratch(M * 256, torch.bfloat16)
    Z = scratch(M * 2 * Ch)
    _lib.check(lib.fwn_tail_train(C.byref(d), o.data_ptr(), M * 256, pa.data_ptr(), pb.data_ptr(), part.data_ptr(), M,
                                  S.data_ptr(), Us.data_ptr(), Z.data_ptr(), stream()), "fwn_tail_train")
    torch.cuda.synchronize()
    assert guard_intact(pa, M * Ch) and guard_intact(pb, M * Ch) and guard_intact(part, nb)
    assert guard_intact(S, M * 256) and guard_intact(Us, M * 256) and guard_intact(Z, M * 2 * Ch)
    return pa, pb, part, S, Us, Z


def zero_scale(full, Ch):
    """The power of two that brings the rms of (U Wzero^T) ez to about 0.5 (|log_s| then reaches 1 to 3 around its centre 0.75),
    from one small forward run with the stock kernels; every case asserts the range it actually gets."""
    if Ch not in ZERO_SCALE:
        hp, model, _ = full
        lib = _lib.load()
        blk, M = Ch.bit_length() - 1, 64
        d = flow_copy(model, hp, blk)
        ez, bz, keep = zero_operands(model, hp, d, Ch, 1.0, np.random.default_rng(Ch))
        o, xa, xb = tail_inputs(hp.n_layer, M, Ch, 5)
        Z = tail_forward_train(d, o, xa, xb, M, Ch, int(lib.fwn_tail_partials(M)))[5]
        ls = (host(Z, (M, 2 * Ch)).astype(np.float64)[:, :Ch] - ez_planes(bz, Ch)[0]) * ez_planes(ez, Ch)[0]       # the part Wzero scales
        rms = float(np.sqrt((ls ** 2).mean()))
        assert np.isfinite(rms) and rms > 0
        ZERO_SCALE[Ch] = 2.0 ** round(np.log2(0.5 / rms))
    return ZERO_SCALE[Ch]


@pytest.mark.parametrize("form,M,Ch,stream_kept", TAIL_CASES, ids=["%s-M%d-ch%d" % c[:3] for c in TAIL_CASES])
def test_tail_epilogue_every_form_both_directions(full, form, M, Ch, stream_kept):
    """ActNorm + affine coupling + log-det partials as tail_zero_prob.h (TAIL_SPLIT3), tail_chain.h (split-chain, fused 128 /
    256) and tail_rs.h (TAIL_RS, 1 / 2 / 4 row tiles) each write them, with 1, 2 and 4 ZeroConv pair tiles.
    Forward (fwn_tail_train, which returns Z): planes and sum(partial) against ref_tail_epilogue on the device's own Z; the
    slots past the exact count keep their zero; fwn_tail gives the same bits.  Inverse (fwn_tail on the forward's output
    planes, same o, so the same Z): planes against the reference, the round trip back to the input planes, and partial -
    "forward only" in fwn.h - still sums to the zero it was given, its guard untouched."""
    hp, model, _ = full
    lib = _lib.load()
    L, blk, npt = hp.n_layer, Ch.bit_length() - 1, npt_of(Ch)
    d = flow_copy(model, hp, blk)
    assert d.npt == npt and d.Ch == Ch and (bool(d.Wts) == (npt == 1))
    if not stream_kept:
        d.Wts = None
    have_stream = bool(d.Wts)
    assert tail_form(M, L, Ch, npt, have_stream)[0] == form
    rng = np.random.default_rng(M * 131 + Ch)
    ez, bz, keep = zero_operands(model, hp, d, Ch, zero_scale(full, Ch), rng)
    an = model._packed.an[(blk, 0)].cpu().numpy()
    nb, nslot = int(lib.fwn_tail_partials(M)), int(lib.fwn_tail_partials_desc(C.byref(d), M, -1))
    assert nb == tail_partials_bound(M) and nslot == tail_slots(M, L, Ch, npt, have_stream) <= nb
    o, xa, xb = tail_inputs(L, M, Ch, M + Ch)
    o0 = o.clone()
    x_a, x_b = xa.cpu().numpy().reshape(M, Ch), xb.cpu().numpy().reshape(M, Ch)

    pa, pb, part, S, Us, Z = tail_forward_train(d, o, xa, xb, M, Ch, nb)
    Zh = host(Z, (M, 2 * Ch))
    assert np.isfinite(Zh).all()
    ref = ref_tail_epilogue(Zh, ez_planes(ez, Ch), an, x_a, x_b, 0)
    ls_var = (Zh[:, :Ch].astype(np.float64) - ez_planes(bz, Ch)[0]) * ez_planes(ez, Ch)[0]                          # log_s without its bias
    ls_rms, ls_max = float(np.sqrt((ls_var ** 2).mean())), float(np.abs(ref["ls"]).max())
    assert 0.2 <= ls_rms <= 1.0 and 1.0 <= ls_max <= 8.0, (ls_rms, ls_max)
    key = "tail %s npt%d" % (form, npt)
    oa, ob = host(pa, (M, Ch)), host(pb, (M, Ch))
    note_ratio(key + " fwd a", oa, ref["oa"], 1e-5 * max(1.0, np.abs(ref["oa"]).max()), "M %d Ch %d" % (M, Ch))
    note_ratio(key + " fwd b", ob, ref["ob"], 1e-5 * max(1.0, np.abs(ref["ob"]).max()), "M %d Ch %d" % (M, Ch))
    ph = host(part, (nb,)).astype(np.float64)
    assert (ph[nslot:] == 0).all(), "slots past the exact count were written"
    note_ratio(key + " logdet", np.array([ph.sum()]), np.array([ref["logdet_sum"]]), np.array([1e-4 * max(1.0, ref["logdet_abs"])]),
               "M %d Ch %d" % (M, Ch))

    # fwn_tail on the same inputs: the same bits
    qa, qb, part2 = plane_dev(xa), plane_dev(xb), dev(np.zeros(nb, np.float32))
    scr = scratch(2 * M * 256, torch.bfloat16)
    _lib.check(lib.fwn_tail(C.byref(d), o.data_ptr(), qa.data_ptr(), qb.data_ptr(), part2.data_ptr(), M, 0, scr.data_ptr(), stream()), "fwn_tail")
    torch.cuda.synchronize()
    assert guard_intact(qa, M * Ch) and guard_intact(qb, M * Ch) and guard_intact(part2, nb) and guard_intact(scr, 2 * M * 256)
    for name, got_t, want_t, shape in (("plane a", qa, pa, (M, Ch)), ("plane b", qb, pb, (M, Ch)), ("partial", part2, part, (nb,))):
        diff = bits32(host(got_t, shape)) != bits32(host(want_t, shape))
        assert not diff.any(), "fwn_tail and fwn_tail_train differ in %s: %d of %d elements, rows %s" % (
            name, int(diff.sum()), diff.size, np.unique(np.nonzero(diff)[0])[:12])

    # inverse, from the forward's output planes
    part3 = dev(np.zeros(nb, np.float32))
    _lib.check(lib.fwn_tail(C.byref(d), o.data_ptr(), qa.data_ptr(), qb.data_ptr(), part3.data_ptr(), M, 1, scr.data_ptr(), stream()), "fwn_tail")
    torch.cuda.synchronize()
    assert guard_intact(qa, M * Ch) and guard_intact(qb, M * Ch) and guard_intact(part3, nb) and guard_intact(scr, 2 * M * 256)
    assert bool((part3[:nb] == 0).all()), "the inverse direction has no log-det: the zeroed partials must still sum to zero"
    inv = ref_tail_epilogue(Zh, ez_planes(ez, Ch), an, oa, ob, 1)
    ia, ib = host(qa, (M, Ch)), host(qb, (M, Ch))
    note_ratio(key + " inv a", ia, inv["oa"], 1e-5 * max(1.0, np.abs(inv["oa"]).max()), "M %d Ch %d" % (M, Ch))
    note_ratio(key + " inv b", ib, inv["ob"], 1e-5 * max(1.0, np.abs(inv["ob"]).max()), "M %d Ch %d" % (M, Ch))
    note_ratio(key + " round trip", np.stack([ia, ib]), np.stack([x_a, x_b]).astype(np.float64),
               2e-5 * max(1.0, float(np.abs(np.stack([x_a, x_b])).max())), "M %d Ch %d" % (M, Ch))
    assert torch.equal(o.view(torch.int16), o0.view(torch.int16)) and all(guard_intact(t, n) for t, n in keep)
    print("tail %-12s M %5d Ch %3d  |ls| rms %.2f max %.2f  " % (form, M, Ch, ls_rms, ls_max)
          + "  ".join("%s %.3f" % (k[len(key) + 1:], v) for k, v in sorted(RATIOS.items()) if k.startswith(key + " ")))


# =================================================================== the table
EXPECTED = ({"res %s" % f for f in RES_ROWS} | {"front %s ch%d" % (f[4], f[0]) for f in FRONT_FORMS}
            | {"tail %s npt%d %s" % (c[0], npt_of(c[2]), w) for c in TAIL_CASES
               for w in ("fwd a", "fwd b", "logdet", "inv a", "inv b", "round trip")})


def test_zz_report_worst_ratios(request):
    """Not a check of its own: prints the worst err / bound of the bounded cases that ran in this session, per stage and
    form; when the whole file ran, every form must be in the table."""
    for k in sorted(RATIOS):
        print("worst err / bound  %-40s %.3f" % (k, RATIOS[k]))
    assert all(v <= 1.0 for v in RATIOS.values())
    if RATIOS and not request.config.getoption("keyword") and not request.config.getoption("deselect", None):
        assert not (EXPECTED - set(RATIOS)), sorted(EXPECTED - set(RATIOS))
