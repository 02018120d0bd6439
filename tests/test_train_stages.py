"""The backward-pass stage kernels, one by one, through the C ABI against plain NumPy fp64 references of their contracts
in include/fwn.h (the references themselves are proved on the CPU in tests/test_train_stage_refs.py).

These kernels take fp32, write fp32 and sum in fp64 in a fixed order, so their tolerances are derived, not measured:
with u = 2^-24, products of fp32 values are exact in fp64 and an fp64 sum of them is exact next to u; what remains is
one fp32 rounding per stored partial and one per output, each at most u times the sum of the absolute terms it covers:
    |got - want| <= 4 u sum|terms|                    (fixed-order fp64 reductions; the factor 2 is head-room for u^2)
    |got - want| <= 2 (6 s) u sum|terms|              (up_dx: an fmaf chain of at most 6 s terms in fp32)
    |got - want| <= 2^-8 |want| + 4 u |want|          (bf16 casts of a short fp32 expression)
`sum|terms|` is the reference's own sum taken over absolute values, per output element.  Every output and scratch buffer
is followed by a guard region of a sentinel that must come back untouched, and the scratch itself starts as NaN: a
partial that is read without having been written shows in the result."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import _lib, packing
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd.model import FloWaveNet

from test_train_stage_refs import ref_small_grads, ref_upsample_bwd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U2 = 2.0 * U * (1.0 + U)       # two dependent fp32 roundings of quantities bounded by the same magnitude
GUARD, SENT = 128, -7.5        # guard elements behind every buffer (>= the widest row any kernel here addresses), their value


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, guard=GUARD):
    """NumPy array -> flat device tensor followed by `guard` sentinel elements."""
    a = np.ascontiguousarray(a)
    if guard == 0:                                        # index tables
        return torch.from_numpy(a.reshape(-1)).cuda()
    t = torch.full((a.size + guard,), SENT, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda")
    t[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return t


def scratch(n, dtype=torch.float32):
    """n NaNs (scratch the kernel must write before it reads) followed by the guard."""
    t = torch.full((int(n) + GUARD,), SENT, dtype=dtype, device="cuda")
    t[:int(n)] = float("nan")
    return t


def host(t, shape):
    return t[:int(np.prod(shape))].cpu().numpy().reshape(shape)


def guard_intact(t, n):
    return t.numel() == int(n) + GUARD and bool((t[int(n):] == SENT).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)          # also catches NaN
    assert not bad.any(), "%s: %d of %d outside the bound; worst err / bound %.3g at %s (got %r want %r)" % (
        what, int(bad.sum()), bad.size, float(np.nanmax(err / np.maximum(bound, 1e-300))), np.unravel_index(np.argmax(bad), bad.shape),
        got[np.unravel_index(np.argmax(bad), bad.shape)], want[np.unravel_index(np.argmax(bad), bad.shape)])


# ------------------------------------------------------------------ 1. fwn_upsample_bwd
# (B, H, W, s, chunks of (b, i) rows the weight-gradient pass must split into)
@pytest.mark.parametrize("B,H,W,s,chunks", [
    (1, 3, 8, 2, 1),          # one chunk, edge taps dominate
    (2, 5, 80, 4, 1),         # small multi-clip
    (1, 64, 7, 4, 4),         # B H = 64: the first size with more than one chunk; odd W below the 8-wide unroll
    (3, 40, 80, 16, 7),       # the real s; 7 chunks of 18 rows over 120: the last one is short
    (13, 80, 80, 4, 64),      # 1040 rows -> 64 chunks of 17: the last two are empty
])
def test_upsample_backward_matches_fp64_reference(B, H, W, s, chunks):
    """up_dpre / up_dx / up_dw / colsum_final: dy in place is dpre exactly, dx and (dwk | dbias) within the derived bounds,
    identical bits on a repeat and with dx = NULL, nothing written outside the buffers."""
    lib = _lib.load()
    rng = np.random.default_rng(B * 100000 + H * 1000 + W * 10 + s)
    x = rng.standard_normal((B, H, W)).astype(np.float32)
    wk = (rng.standard_normal((2 * s, 3)) * 0.3).astype(np.float32)
    y = rng.standard_normal((B, H * s, W)).astype(np.float32)
    zeros = rng.random(y.shape)
    y[zeros < 0.05] = 0.0                                 # LeakyReLU'(0) = 0.4: y > 0, not y >= 0
    y[zeros > 0.98] = -0.0
    dy = rng.standard_normal((B, H * s, W)).astype(np.float32)
    ref = ref_upsample_bwd(dy, y, x, wk, s)
    npart = int(lib.fwn_upsample_bwd_partials(B, H, s))
    assert npart == chunks * (6 * s + 1)
    d_y, d_x, d_wk = dev(y), dev(x), dev(wk)

    def run(with_dx):
        d_dy, d_dx, d_dw, d_part = dev(dy), scratch(x.size), scratch(6 * s + 1), scratch(npart)
        _lib.check(lib.fwn_upsample_bwd(d_dy.data_ptr(), d_y.data_ptr(), d_x.data_ptr(), B, H, W, s, d_wk.data_ptr(),
                                        d_dx.data_ptr() if with_dx else None, d_dw.data_ptr(), d_part.data_ptr(), stream()), "fwn_upsample_bwd")
        torch.cuda.synchronize()
        assert guard_intact(d_dy, dy.size) and guard_intact(d_dx, x.size) and guard_intact(d_dw, 6 * s + 1) and guard_intact(d_part, npart)
        if not with_dx:
            assert bool(torch.isnan(d_dx[:x.size]).all())                  # dx = NULL: nothing of it is touched
        return host(d_dy, dy.shape), host(d_dx, x.shape), host(d_dw, (6 * s + 1,))

    dpre, dx, dw = run(True)
    assert same_bits(dpre, ref["dpre"])
    assert_within(dx, ref["dx"], 2.0 * (6 * s) * U * ref["dx_abs"], "dx")
    assert_within(dw, ref["dwk_bias"], 4.0 * U * ref["dwk_bias_abs"], "dwk_bias")
    dpre2, dx2, dw2 = run(True)
    assert same_bits(dpre2, dpre) and same_bits(dx2, dx) and same_bits(dw2, dw)
    dpre3, _, dw3 = run(False)
    assert same_bits(dpre3, dpre) and same_bits(dw3, dw)
    assert same_bits(host(d_y, y.shape), y) and same_bits(host(d_x, x.shape), x) and same_bits(host(d_wk, wk.shape), wk)


# ------------------------------------------------------------------ 2. fwn_flow_small_grads
def actnorm_table(rng, ch):
    """[2][4][Ch] = (shift, scale = exp(.), 1 / scale, 3 logs) as tests/test_train.py builds it."""
    an = rng.standard_normal((2, 4, ch)).astype(np.float32) * np.float32(0.3)
    an[:, 1] = np.exp(an[:, 1])
    an[:, 2] = np.float32(1.0) / an[:, 1]
    return an


# (M, Ch, workgroups of the first pass)
@pytest.mark.parametrize("M,Ch,blocks", [
    (3, 1, 1),            # one block, fewer elements than threads
    (5000, 1, 9),         # 9 blocks; the LDS fold runs all 8 halvings
    (333, 8, 5),          # mid-size Ch, uneven row count
    (700, 64, 87),        # the ZeroConv fold (period 2 Ch = 128) stops one step before the others (period 64)
    (64, 128, 16),        # exactly one 16-wide batch of the final pass
    (68, 128, 17),        # one past it
    (385, 128, 96),       # capped at 96 blocks of 5 rows: blocks 77 - 95 own no rows and must contribute exact zeros
    (1, 128, 1),          # a single row
])
def test_flow_small_grads_match_fp64_reference(M, Ch, blocks):
    """flow_small_grads_kernel + its final pass: db, dlogs, dzscale within the reduction bound, the four planes within
    the bound of their one or two fp32 operations, identical bits on a repeat, scratch guard untouched."""
    lib = _lib.load()
    rng = np.random.default_rng(M * 1000 + Ch)
    ga, ya, gb, yb = (rng.standard_normal((M, Ch)).astype(np.float32) for _ in range(4))
    dzz = rng.standard_normal((M, 2 * Ch)).astype(np.float32)
    an = actnorm_table(rng, Ch)
    br, zc = rng.permutation(Ch).astype(np.int64), rng.permutation(2 * Ch).astype(np.int64)
    ref = ref_small_grads(ga, ya, gb, yb, dzz, an, br, zc)
    npart = int(lib.fwn_flow_small_grads_partials(M, Ch))
    assert npart == blocks * 6 * Ch
    d_an, d_dzz, d_br, d_zc = dev(an), dev(dzz), dev(br, 0), dev(zc, 0)

    def run():
        planes = [dev(a) for a in (ga, ya, gb, yb)]
        outs = [scratch(2 * Ch) for _ in range(3)]
        part = scratch(npart, torch.float64)
        _lib.check(lib.fwn_flow_small_grads(*[p.data_ptr() for p in planes], d_dzz.data_ptr(), d_an.data_ptr(), M, Ch, d_br.data_ptr(),
                                            d_zc.data_ptr(), part.data_ptr(), *[o.data_ptr() for o in outs], stream()), "fwn_flow_small_grads")
        torch.cuda.synchronize()
        assert all(guard_intact(p, M * Ch) for p in planes) and all(guard_intact(o, 2 * Ch) for o in outs) and guard_intact(part, npart)
        assert not bool(torch.isnan(part[:npart]).any())                      # every block wrote its slot, the empty ones too
        return [host(p, (M, Ch)) for p in planes], [host(o, (2 * Ch,)) for o in outs]

    (g0, x0, g1, x1), (db, dlogs, dzs) = run()
    assert_within(db, ref["db"], 4.0 * U * ref["db_abs"], "db")
    assert_within(dlogs, ref["dlogs"], 4.0 * U * ref["dlogs_abs"], "dlogs")
    assert_within(dzs, ref["dzscale"], 4.0 * U * ref["dzscale_abs"], "dzscale")
    assert_within(g0, ref["g0"], U2 * np.abs(ref["g0"]), "ga")              # one multiply
    assert_within(g1, ref["g1"], U2 * np.abs(ref["g1"]), "gb")
    assert_within(x0, ref["x0"], U2 * ref["x0_abs"], "ya")                  # a multiply, then a subtraction
    assert_within(x1, ref["x1"], U2 * ref["x1_abs"], "yb")
    planes2, outs2 = run()
    assert all(same_bits(a, b) for a, b in zip(planes2 + outs2, [g0, x0, g1, x1, db, dlogs, dzs]))
    assert same_bits(host(d_dzz, dzz.shape), dzz) and same_bits(host(d_an, an.shape), an)


# ------------------------------------------------------------------ 3. element-wise and reduction entries
@pytest.mark.parametrize("Ch", [1, 8, 128])
def test_actnorm_apply_and_backward_single_plane(Ch):
    """fwn_actnorm_apply (one plane) and fwn_actnorm_bwd at n = 37 Ch (never a multiple of 256), and the round trip:
    apply, then bwd on the result, gives x back to five roundings (x + shift, times scale, 1 / scale in the table,
    times it, minus shift), each relative to at most |x| + |shift|: 6 u (|x| + |shift|) with the second-order terms."""
    lib = _lib.load()
    rng = np.random.default_rng(Ch)
    M = 37
    n = M * Ch
    assert n % 256 != 0
    an = actnorm_table(rng, Ch)[1]                        # the second plane's table: a pointer into the flow's
    x = rng.standard_normal((M, Ch)).astype(np.float32)
    g = rng.standard_normal((M, Ch)).astype(np.float32)
    x64, g64, a64 = x.astype(np.float64), g.astype(np.float64), an.astype(np.float64)
    d_an, d_x, d_g = dev(an), dev(x), dev(g)
    _lib.check(lib.fwn_actnorm_apply(d_x.data_ptr(), d_an.data_ptr(), n, Ch, stream()), "fwn_actnorm_apply")
    torch.cuda.synchronize()
    y = host(d_x, (M, Ch)).copy()
    assert_within(y, (x64 + a64[0]) * a64[1], U2 * (np.abs(x64) + np.abs(a64[0])) * a64[1], "actnorm_apply")
    _lib.check(lib.fwn_actnorm_bwd(d_g.data_ptr(), d_x.data_ptr(), d_an.data_ptr(), n, Ch, stream()), "fwn_actnorm_bwd")
    torch.cuda.synchronize()
    back, dx = host(d_x, (M, Ch)), host(d_g, (M, Ch))
    y64 = y.astype(np.float64)
    assert_within(dx, g64 * a64[1], U2 * np.abs(g64 * a64[1]), "actnorm_bwd dy")
    assert_within(back, y64 * a64[2] - a64[0], U2 * (np.abs(y64 * a64[2]) + np.abs(a64[0])), "actnorm_bwd y")
    assert_within(back, x64, 6.0 * U * (np.abs(x64) + np.abs(a64[0])), "round trip")
    assert guard_intact(d_x, n) and guard_intact(d_g, n) and same_bits(host(d_an, an.shape), an)


# (M, C, row blocks of the first pass)
@pytest.mark.parametrize("M,C,blocks", [
    (1, 1, 1),                # minimum
    (3, 2, 1),                # fewer rows than the 4 row-parts
    (511, 72, 1),             # one block; C not a multiple of 64
    (513, 72, 2),             # two blocks of 257 and 256 rows
    (1281, 300, 5),           # 5 blocks; 5 column groups, the last one ragged
    (70000, 256, 256),        # block count capped by 1024 / ceil(C / 64)
])
def test_colsum_prod_matches_fp64_reference(M, C, blocks):
    """fwn_colsum_prod with B and with B = NULL, scale != 1: out[c] = scale sum_m A B within 4 u |scale| sum_m |A B|."""
    lib = _lib.load()
    rng = np.random.default_rng(M + C)
    A, Bm = rng.standard_normal((M, C), dtype=np.float32), rng.standard_normal((M, C), dtype=np.float32)
    scale = -1.75
    npart = int(lib.fwn_colsum_partials(M, C))
    assert npart == blocks * C
    d_A, d_B = dev(A), dev(Bm)
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    for with_b in (True, False):
        terms = A64 * B64 if with_b else A64
        want, want_abs = scale * terms.sum(0), abs(scale) * np.abs(terms).sum(0)
        res = []
        for rep in range(2):
            part, out = scratch(npart), scratch(C)
            _lib.check(lib.fwn_colsum_prod(d_A.data_ptr(), d_B.data_ptr() if with_b else None, M, C, scale, part.data_ptr(), out.data_ptr(),
                                           stream()), "fwn_colsum_prod")
            torch.cuda.synchronize()
            assert guard_intact(part, npart) and guard_intact(out, C) and not bool(torch.isnan(part[:npart]).any())
            res.append(host(out, (C,)))
        assert_within(res[0], want, 4.0 * U * want_abs, "colsum_prod (B %s)" % ("given" if with_b else "NULL"))
        assert same_bits(res[0], res[1])
    assert guard_intact(d_A, A.size) and guard_intact(d_B, Bm.size)


def bf16_dev(a, guard_rows=0, cols=None):
    """fp32 array [M][cols] -> bf16 device tensor [M + guard_rows][cols], guard rows = SENT."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = torch.full((a.shape[0] + guard_rows, a.shape[1]), SENT, dtype=torch.bfloat16, device="cuda")
    t[:a.shape[0]] = torch.from_numpy(a).cuda().to(torch.bfloat16)
    return t


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("M", [1, 333])
@pytest.mark.parametrize("ld_do", [256, 512])
def test_gate_bwd_matches_the_formula(M, ld_do):
    """fwn_gate_bwd against (do sg (1 - tf^2) | do tf sg (1 - sg)) on its own bf16 inputs - the kernel that
    test_gemm_gate_derivative_epilogue_equals_store_then_gate_bwd takes as its reference.  ld_do = 512: do is the upper
    column block of a wider matrix.  Output: the bf16 cast of an fp32 expression of at most four roundings."""
    lib = _lib.load()
    rng = np.random.default_rng(M + ld_do)
    wide = bf16_dev(rng.standard_normal((M, ld_do)), guard_rows=1)
    aux = bf16_dev(np.concatenate([np.tanh(2.0 * rng.standard_normal((M, 256))), 1 / (1 + np.exp(-2.0 * rng.standard_normal((M, 256))))], 1), guard_rows=1)
    dpre = torch.full((M + 8, 512), SENT, dtype=torch.bfloat16, device="cuda")
    do_ptr = wide.data_ptr() + 2 * (ld_do - 256)
    _lib.check(lib.fwn_gate_bwd(do_ptr, ld_do, aux.data_ptr(), M, dpre.data_ptr(), stream()), "fwn_gate_bwd")
    torch.cuda.synchronize()
    d, tf, sg = f64(wide[:M, ld_do - 256:]), f64(aux[:M, :256]), f64(aux[:M, 256:])
    want = np.concatenate([d * sg * (1 - tf * tf), d * tf * sg * (1 - sg)], 1)
    assert_within(f64(dpre[:M]), want, (2.0 ** -8 + 4.0 * U) * np.abs(want), "dpre")
    assert bool((dpre[M:] == SENT).all())


@pytest.mark.parametrize("n", [1, 1023, 1024, 8191, 8192, 8193, 20000])
def test_prior_logp_either_side_of_its_unroll(n):
    """fwn_prior_logp: log_p = 0.5 (-log 2 pi - mean z^2), logdet = sum(partial) / n, for n and n_partial on both sides of
    the 8 x 1024 unrolled loops; fp64 sums and one cast: 1e-6 relative."""
    lib = _lib.load()
    rng = np.random.default_rng(n)
    z = rng.standard_normal(n).astype(np.float32)
    d_z = dev(z)
    for n_partial in (0, 3, 8200):
        part = (rng.standard_normal(n_partial) + 0.5).astype(np.float32)
        d_p, out2 = dev(part), scratch(2)
        _lib.check(lib.fwn_prior_logp(d_z.data_ptr(), n, d_p.data_ptr() if n_partial else None, n_partial, out2.data_ptr(), stream()), "fwn_prior_logp")
        torch.cuda.synchronize()
        got = host(out2, (2,)).astype(np.float64)
        want_lp = 0.5 * (-np.log(2.0 * np.pi) - (z.astype(np.float64) ** 2).mean())
        want_ld = part.astype(np.float64).sum() / n
        assert abs(got[0] - want_lp) <= 1e-6 * abs(want_lp), (n, n_partial, got[0], want_lp)
        assert abs(got[1] - want_ld) <= 1e-6 * abs(want_ld), (n, n_partial, got[1], want_ld)
        assert guard_intact(out2, 2) and guard_intact(d_p, n_partial)
    assert guard_intact(d_z, n)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 3 * 2 ** 20 + 1])
def test_grad_norm_tails_and_blocks(n):
    """fwn_grad_norm = ||g gscale||_2: the float4 body and its scalar tail, one block and the grid-stride loop of the
    capped 2048 blocks; gscale != 1; fp64 sums and one cast: 1e-6 relative."""
    lib = _lib.load()
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n, dtype=np.float32)
    gscale = 1.0 / 192.0
    nb = int(lib.fwn_grad_norm_partials(n))
    assert nb == min(2048, (n + 1023) // 1024)
    d_g, part, out = dev(g), scratch(nb, torch.float64), scratch(1)
    assert d_g.data_ptr() % 16 == 0
    _lib.check(lib.fwn_grad_norm(d_g.data_ptr(), n, gscale, part.data_ptr(), out.data_ptr(), stream()), "fwn_grad_norm")
    torch.cuda.synchronize()
    want = float(np.sqrt((g.astype(np.float64) ** 2).sum())) * float(np.float32(gscale))
    got = float(host(out, (1,))[0])
    assert abs(got - want) <= 1e-6 * want, (got, want)
    assert guard_intact(part, nb) and guard_intact(out, 1) and guard_intact(d_g, n) and not bool(torch.isnan(part[:nb]).any())


# ------------------------------------------------------------------ 4. fwn_gate_train: o and aux in every form
@pytest.fixture(scope="module")
def full_packed():
    """The parameters of tests/test_gpu_parity.py's full_model fixture, packed; no data-dependent init (the gate has none)."""
    hp = default_hparams()
    params = W.synthetic_params(hp, 1234)
    model = FloWaveNet(hp).load_params(params)
    p64 = {}
    for blk in (0, 1):                                    # the gate's own parameters of flow 0 of blocks 0 and 1, fp64
        pre = W.flow_prefix(blk, 0) + "/WaveNet/ResBlock_"
        p64.update({k: np.asarray(v, np.float64) for k, v in params.items() if k.startswith(pre)})
    return hp, model, p64


def gate_form(m, dil, hoisted):
    """Which kernel fwn_launch_gate (csrc/flow_kernels.hip) picks for a training gate (aux given: never the
    register-streamed one) - restated so that every case asserts the branch it is there for."""
    t256, t128 = (m + 255) // 256, (m + 127) // 128
    if dil <= 3 and t256 * 4 >= 192:
        return "halo256x256" if t256 * 2 >= 192 else "halo256x128"
    if dil <= 3 and t128 * 4 >= 192:
        return "halo128x128"
    # launch_ring, N = 512, FILL = 192; the smallest tile splits K inside the workgroup and prefetches P (PRE epilogue)
    if t256 * 2 >= 192 or t256 * 4 >= 192 or t128 * 4 >= 192:
        return "ring-big"
    return "ring64x128" if ((m + 63) // 64) * 4 >= 192 else "ring64x64-pre"


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("blk,b,ti,hoisted,form", [
    (0, 3, 100, False, "ring64x64-pre"),
    (0, 7, 1000, False, "halo128x128"),
    (0, 13, 1000, False, "halo256x128"),
    (0, 26, 1000, False, "halo256x256"),      # block 0 of the training shape: the tap-sharing tiles with the aux stores
    (1, 7, 1000, False, "halo128x128"),       # cin = 160
    # hoisted (P from fwn_cond), where csrc/train_api.hip passes P: below 4096 rows.  One ring-sized case per epilogue variant
    (0, 3, 100, True, "ring64x64-pre"),       # P prefetched ahead of the K loop (PRE)
    (0, 4, 800, True, "ring64x128"),          # P loaded in the epilogue (non-PRE): 3009 .. 4095 rows
])
def test_gate_train_o_and_aux_match_oracle(full_packed, blk, b, ti, hoisted, form, layer):
    """fwn_gate_train against the oracle's ResBlock gate (modules.py:113-124; the expression of
    test_gate_stage_kernel_matches_oracle): o = tanh(f) sigmoid(g) and aux = (tanh f | sigmoid g) in natural channel
    order, each a bf16 value in (-1, 1) computed from bf16 weights - the existing test's tolerances for each of the three.
    o against its own factors: o = bf16(tf sg) of the fp32 factors, aux their bf16 casts.  With tf = a 2^p, sg = b 2^q,
    a, b in [1, 2), a cast moves a mantissa by at most half a bf16 ulp = 2^-8, so aux_tf aux_sg is off by (a + b) 2^-8 and o
    by 2^-8 (a b < 2, ulp 2^-7: (a + b + 1) / 2 < 2 ulps, as a + b < 3 there) or 2^-7 (a b >= 2, ulp 2^-6: at most 1.5 ulps).
    The ulp is that of the exact product's binade; o never lies below it, the product of the rounded factors may (a b just
    above 2), so it is taken from the larger of the two values compared.  Eight guard rows behind row M of o and aux stay
    untouched (the partial last tile relies on buffer-descriptor bounds)."""
    hp, model, p64 = full_packed
    lib = _lib.load()
    d = model._packed.flow_descs[blk * hp.n_flow]
    m, half, L = b * ti, hp.num_mels // 2, hp.n_layer
    assert gate_form(m, 3 ** layer, hoisted) == form and (not hoisted or m < 4096) and d.cin == half * (2 << blk)
    rng = np.random.default_rng(blk * 1000 + b * 10 + layer + 500 * hoisted)
    h = bf16_dev(rng.standard_normal((m, 256)) * 0.5)
    ca = bf16_dev(rng.random((m, d.cin)))
    o, aux = bf16_dev(np.zeros((m, 256)), 8), bf16_dev(np.zeros((m, 512)), 8)
    o[:m], aux[:m] = float("nan"), float("nan")
    P = None
    if hoisted:
        P = torch.full((L, m, 512), float("nan"), device="cuda")
        _lib.check(lib.fwn_cond(ca.data_ptr(), d.Wc[0], P.data_ptr(), 512 * d.kcpad, m * 512, 0, 1, 1, L, m, d.cin, d.kcpad, stream()), "fwn_cond")
    _lib.check(lib.fwn_gate_train(C.byref(d), layer, h.data_ptr(), None if hoisted else ca.data_ptr(), P[layer].data_ptr() if hoisted else None,
                                  o.data_ptr(), aux.data_ptr(), m, ti, stream()), "fwn_gate_train")
    torch.cuda.synchronize()
    assert bool((o[m:] == SENT).all()) and bool((aux[m:] == SENT).all())
    src = packing.cond_src_k(blk, half)[:d.cin]           # device K order of c_a -> the reference's channel order
    c_log = np.empty((b, ti, d.cin))
    c_log[:, :, src] = f64(ca).reshape(b, ti, d.cin)
    h64 = f64(h).reshape(b, ti, 256)
    rp = W.flow_prefix(blk, 0) + "/WaveNet/ResBlock_%d" % layer
    f = onp.conv_layer(p64, rp + "/Conv_filter", h64, 3, 3 ** layer) + onp.conv1x1(p64, rp + "/filter_conv_c", c_log)
    g = onp.conv_layer(p64, rp + "/Conv_gate", h64, 3, 3 ** layer) + onp.conv1x1(p64, rp + "/gate_conv_c", c_log)
    tf, sg = np.tanh(f).reshape(m, 256), onp.sigmoid(g).reshape(m, 256)
    got_o, got_tf, got_sg = f64(o[:m]), f64(aux[:m, :256]), f64(aux[:m, 256:])
    worst = {}
    for name, got, want in (("o", got_o, tf * sg), ("aux tanh", got_tf, tf), ("aux sigmoid", got_sg, sg)):
        err = np.abs(got - want)
        worst[name] = (float(np.nanmax(err)), float(err.mean()))
    prod = got_tf * got_sg
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(prod), np.abs(got_o)), 2.0 ** -126))) - 7)
    self_err = np.abs(got_o - prod) / ulp
    print("gate_train blk %d M %d layer %d %s %s: " % (blk, m, layer, "hoisted" if hoisted else "fused", form)
          + "  ".join("%s max %.3e mean %.3e" % (k, v[0], v[1]) for k, v in worst.items())
          + "  |o - tf sg| max %.2f ulp" % float(np.nanmax(self_err)))
    for name, (emax, emean) in worst.items():
        # bf16 weights and a bf16 output in (-1, 1): half an output ulp is 2e-3, the weight rounding adds ~1e-2
        assert emax < 3e-2 and emean < 2e-3, (name, emax, emean)
    assert bool((self_err <= 2.0).all()), float(np.nanmax(self_err))
