"""Plain NumPy fp64 references of three inference stages - the front conv (fwn_front), the residual 1x1 (fwn_res) and the
tail's ActNorm + coupling + log-det epilogue (fwn_tail / fwn_tail_train) - and their proofs against the oracle
(oracle/flowavenet_np.py) on the CPU.  tests/test_infer_stages.py holds the HIP kernels to these references; here the
references themselves are checked, so that the plane-order and logical-order permutations (packing.bitrev_table,
packing.actnorm_table), the (log_s | t) column order of Z and the clip-edge rule of the three taps are not merely assumed.

The module also restates the three dispatch rules of csrc/flow_kernels.hip (fwn_launch_res + fwn_ring_tile_for,
fwn_launch_front, fwn_tail_form) so that every GPU case can assert the form it is there to reach, derives the row counts
of the GPU cases from those rules, and checks the tail rule against the library's own host queries without a GPU."""
import numpy as np
import pytest

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import packing
from tf_flowavenet_amd import weights as W

from conftest import small_hparams
from test_train_gemm_refs import lib, ref_gemm  # noqa: F401  (lib: the fixture that builds the library if it is missing)

SQRT_HALF_F32 = np.float32(0.70710678118654752)     # the constant of ResProb's epilogues, as the fp32 the kernel multiplies by


# ------------------------------------------------------------------ references
def ref_front(xa, an_a, Wf, bias, Ti, apply_an):
    """fwn_front: h0 = ReLU(conv_k3(actnorm?(xa)) + bias) per clip of Ti rows (modules.py:144,164-165).
    xa [M][Ch] (plane order); an_a [4][Ch] = (shift, scale, ..) of the a-plane; Wf [256][>= 3 Ch] with K = tap Ch + tau;
    taps that leave their clip read zero.  Returns (h0 [M][256], terms = sum |x' w| + |bias| with x' the ActNorm-applied x)."""
    xa = np.asarray(xa, np.float64)
    M, Ch = xa.shape
    an_a = np.asarray(an_a, np.float64)
    x = (xa + an_a[0]) * an_a[1] if apply_an else xa
    segs = [(x, Ch, tap - 1, tap * Ch) for tap in range(3)]
    return ref_gemm(segs, Wf, M, 256, Ti=Ti, bias=bias, relu=True)


def ref_res(o, h, Wr, bias):
    """fwn_res: h' = (h + o Wr^T + bias) sqrt(1/2) (modules.py:126-128), sqrt(1/2) as the kernel's fp32 constant.
    o, h [M][256]; Wr [256][256] = [n][k].  Returns (h', terms)."""
    M = np.asarray(o).shape[0]
    return ref_gemm([(o, 256, 0, 0)], Wr, M, 256, bias=bias, R=h, rscale=1.0, oscale=SQRT_HALF_F32)


def ref_tail_epilogue(Z, ez, an, xa, xb, inverse):
    """The arithmetic of TailZeroProb::epilogue_impl (csrc/tail_zero_prob.h; written again in tail_chain.h and tail_rs.h)
    in fp64.  Z [M][2 Ch] = (log_s | t) columns in plane order, before the exp(3 scale) factor ez [2][Ch] = (ez_ls, ez_t);
    an [2][4][Ch] = per plane (shift, scale, 1 / scale, 3 logs); xa, xb [M][Ch].
    Returns dict(oa, ob, ls; forward also logdet_sum = sum_rows sum_tau (a_l3 + b_l3 - ls) and logdet_abs, the same sum
    over the absolute values of its three terms)."""
    Z, xa, xb = (np.asarray(v, np.float64) for v in (Z, xa, xb))
    ez, an = np.asarray(ez, np.float64), np.asarray(an, np.float64)
    M, Ch = xa.shape
    ls, t = Z[:, :Ch] * ez[0], Z[:, Ch:] * ez[1]
    (a_sh, a_sc, a_isc, a_l3), (b_sh, b_sc, b_isc, b_l3) = an[0], an[1]
    if not inverse:
        oa = (xa + a_sh) * a_sc
        ob = ((xb + b_sh) * b_sc - t) * np.exp(-ls)
        return dict(oa=oa, ob=ob, ls=ls, logdet_sum=float((a_l3 + b_l3 - ls).sum()),
                    logdet_abs=float((np.abs(a_l3) + np.abs(b_l3) + np.abs(ls)).sum()))
    ob = (xb * np.exp(ls) + t) * b_isc - b_sh
    oa = xa * a_isc - a_sh
    return dict(oa=oa, ob=ob, ls=ls)


def ez_planes(ezero, Ch):
    """fwn_flow_desc.ezero [npt 64] (row pt 64 + fg 32 + j serves tau = pt 32 + j; fg 0 = log_s, 1 = t) -> [2][Ch]."""
    tau = np.arange(Ch)
    ezero = np.asarray(ezero)
    return np.stack([ezero[(tau // 32) * 64 + tau % 32], ezero[(tau // 32) * 64 + 32 + tau % 32]])


# ------------------------------------------------------------------ the dispatch rules, restated
def ceil_div(a, b):
    return -(-a // b)


def ring_tile_for(M, N, allow256):
    """fwn_ring_tile_for (csrc/fwn_internal.h)."""
    FILL = 192
    if allow256 and N % 256 == 0 and ceil_div(M, 256) * (N // 256) >= FILL:
        return "256x256"
    if ceil_div(M, 256) * (N // 128) >= FILL:
        return "256x128"
    if ceil_div(M, 128) * (N // 128) >= FILL:
        return "128x128"
    if ceil_div(M, 64) * (N // 128) >= FILL:
        return "64x128"
    return "splitk64x64"


def res_form(M):
    """fwn_launch_res: the 128 x 128 tile at ring depth 2 from ceil(M / 256) 2 >= 192 on, else launch_ring(N = 256, 16 k-steps:
    the split-K tile takes 128-wide chunks over 4 wave groups).  launch_ring's 256 x 128 arm has the same condition as the
    depth-2 branch in front of it: unreachable for N = 256."""
    if ceil_div(M, 256) * 2 >= 192:
        return "128x128d2"
    t = ring_tile_for(M, 256, False)
    assert t != "256x128"
    return {"128x128": "128x128d3", "64x128": "64x128", "splitk64x64": "splitk64x64"}[t]


RES_TILE_ROWS = {"splitk64x64": 64, "64x128": 64, "128x128d3": 128, "128x128d2": 128}
RES_RULE_ROWS = {"splitk64x64": 64, "64x128": 64, "128x128d3": 128, "128x128d2": 256}      # the unit the rule counts rows in


def first_rows(form_of, lo=1, hi=70000):
    """form -> the smallest M in [lo, hi) that reaches it."""
    first = {}
    for m in range(lo, hi):
        first.setdefault(form_of(m), m)
    return first


def res_row_counts():
    """form -> row counts of the GPU cases: the first M of the form (a one-row last tile) and the next exact multiple of the
    unit its rule counts in (a multiple of the tile height); the split-K form, which starts at M = 1, also either side of one tile and its last M."""
    first = first_rows(res_form, hi=30000)
    out = {}
    for form, m0 in first.items():
        bm = RES_RULE_ROWS[form]
        out[form] = [m0, ceil_div(m0, bm) * bm]
    out["splitk64x64"] = [1, 63, 64, 65, first["64x128"] - 1]
    return out


def front_form(Ch, have_W2, M):
    """fwn_launch_front for a 16-byte aligned plane (fwn_front refuses any other, so the xprep_kernel + ring form behind the
    first branch is not reachable through the entry point) and no e4m3 side copy."""
    if have_W2 and Ch in (16, 32, 64, 128):
        return "mfma%d" % Ch
    if Ch <= 16:
        kmax = 6 if Ch <= 2 else 12 if Ch <= 4 else 24 if Ch <= 8 else 48
        return "valu_k%d_r%d" % (kmax, 64 if M >= 64 * 512 else 16)
    return "gemm128_%d" % (2 if ceil_div(M, 128) * 2 >= 512 else 1)


TAIL_SPLIT_MAX, TAIL256_MIN, TAIL_SPLIT_CHAIN_MIN = 12288, 192 * 256, 6144
TRS_MIN_ROWS, TRS_ROWS64, TRS_ROWS128, TRS_MAX_ROWS = 1008, 6144, 12288, 49152


def tail_form(M, L, Ch, npt, have_stream):
    """fwn_tail_form -> (kind, rows per workgroup)."""
    if have_stream and L == 2 and npt == 1 and Ch <= 32 and TRS_MIN_ROWS <= M < TRS_MAX_ROWS:
        mt = 4 if M >= TRS_ROWS128 else 2 if M >= TRS_ROWS64 else 1
        return "rs%d" % mt, 32 * mt
    if M > TAIL_SPLIT_MAX:
        return ("fused256", 256) if M >= TAIL256_MIN else ("fused128", 128)
    return ("split_chain", 64) if M >= TAIL_SPLIT_CHAIN_MIN else ("split3", 64)


def tail_slots(M, L, Ch, npt, have_stream):
    """fwn_tail_slots without a chained front conv: the log-det partials one launch writes."""
    kind, rows = tail_form(M, L, Ch, npt, have_stream)
    return ceil_div(M, 64) * 8 if kind == "split3" else ceil_div(M, rows)


def tail_partials_bound(M):
    """fwn_tail_partials: the larger count of the two forms that may serve M rows."""
    return max(tail_slots(M, 2, 1, 1, False), tail_slots(M, 2, 1, 1, True))


def npt_of(Ch):
    return max(1, ceil_div(Ch, 32))


# (form, M, Ch, the descriptor keeps its fragment stream Wts).  Each form at its smallest M of the table in the issue and one
# past it (or one past a tile); TAIL_RS at Ch = 1, 8, 16, 32 because its epilogue evaluates only the register groups that exist.
TAIL_CASES = (
    [("split3", m, ch, True) for m in (63, 65) for ch in (1, 32, 64, 128)]
    + [("split_chain", m, ch, False) for m in (6144, 6145) for ch in (1, 32, 64, 128)]
    + [("fused128", 12289, ch, False) for ch in (8, 32, 64, 128)]
    + [("fused256", m, ch, True) for m in (49152, 49153) for ch in (1, 32, 64, 128)]
    + [("rs%d" % mt, m + o, ch, True) for mt, m in ((1, 1008), (2, 6144), (4, 12288)) for o in (0, 1) for ch in (1, 8, 16, 32)]
)


# ------------------------------------------------------------------ proofs of the references
def plane_order(x, block):
    """Logical channels [B][T][2 Ch] -> the two planes [B T][Ch] in natural (plane) order."""
    ch = 1 << block
    br = packing.bitrev_table(block).astype(np.int64)
    flat = x.reshape(-1, 2 * ch)
    return flat[:, br], flat[:, ch + br]


def tiny_flow(block, seed):
    """fp64 parameters of one flow at `block` (Ch = 2^block) with random ActNorm and a non-trivial ZeroConv scale and bias."""
    hp = small_hparams(n_block=block + 1, n_flow=1)
    p = onp.to_f64(W.synthetic_params(hp, seed, actnorm="random"))
    rng = np.random.default_rng(seed)
    zp = W.flow_prefix(block, 0) + "/WaveNet/ZeroConv1d"
    p[zp + "/scale"] = rng.uniform(-0.1, 0.1, p[zp + "/scale"].shape)
    p[zp + "/bias"] = rng.uniform(-0.1, 0.1, p[zp + "/bias"].shape)
    p[zp + "/kernel"] = p[zp + "/kernel"] * 16.0                # |log_s| of order 1
    return hp, p, W.flow_prefix(block, 0)


def an_table64(p, fp, block):
    """packing.actnorm_table in fp64: the table the device holds is this one rounded to fp32 (asserted), so the proofs can
    use the unrounded one and stay at 1e-12."""
    ch = 1 << block
    br = packing.bitrev_table(block).astype(np.int64)
    b, l3 = p[fp + "/ActNorm/b"].reshape(-1), 3.0 * p[fp + "/ActNorm/logs"].reshape(-1)
    an = np.empty((2, 4, ch))
    for role in range(2):
        idx = role * ch + br
        an[role] = b[idx], np.exp(l3[idx]), np.exp(-l3[idx]), l3[idx]
    assert np.array_equal(an.astype(np.float32), packing.actnorm_table(p[fp + "/ActNorm/b"], p[fp + "/ActNorm/logs"], block))
    return an


@pytest.mark.parametrize("Ti", [1, 2, 7])
@pytest.mark.parametrize("block", [0, 1, 2, 3])
def test_front_reference_equals_the_oracle_conv_behind_actnorm(block, Ti):
    """W and an built from the parameters through packing's own tables (front_src_k: K = tap Ch + tau reads logical channel
    bitrev(tau); actnorm_table): ref_front on the a-plane equals ReLU(Conv_front(ActNorm(x)_a)) of the oracle per clip.
    Clip lengths 1 (only the centre tap survives), 2 and 7."""
    hp, p, fp = tiny_flow(block, 7 + block)
    ch, B = 1 << block, 3
    rng = np.random.default_rng(block * 10 + Ti)
    x = rng.standard_normal((B, Ti, 2 * ch))
    an = an_table64(p, fp, block)
    fold = onp.wn_kernel_1d(p, fp + "/WaveNet/Conv_front").reshape(3 * ch, 256)
    Wf = fold[packing.front_src_k(block)[:3 * ch]].T                       # [256][3 Ch]
    xa, _ = plane_order(x, block)
    for apply_an in (1, 0):
        y = onp.actnorm_forward(p, fp + "/ActNorm", x)[0] if apply_an else x
        want = np.maximum(onp.conv_layer(p, fp + "/WaveNet/Conv_front", y[:, :, :ch], 3, 1), 0.0).reshape(B * Ti, 256)
        got, terms = ref_front(xa, an[0], Wf, p[fp + "/WaveNet/Conv_front/bias"], Ti, apply_an)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert (got <= terms + 1e-12).all() and (got > 0).any()


def test_res_reference_equals_the_oracle_res_block():
    """ref_res on the oracle's own gate output o = tanh(f) sigmoid(g) equals the first return value of onp.res_block, up to
    the ratio of the kernel's fp32 sqrt(1/2) to the oracle's fp64 one (2^-26 relative, taken out before comparing)."""
    hp, p, fp = tiny_flow(0, 3)
    rp = fp + "/WaveNet/ResBlock_0"
    rng = np.random.default_rng(1)
    B, T = 2, 9
    h, c = rng.standard_normal((B, T, 256)), rng.random((B, T, hp.num_mels))
    f = onp.conv_layer(p, rp + "/Conv_filter", h, 3, 1) + onp.conv1x1(p, rp + "/filter_conv_c", c)
    g = onp.conv_layer(p, rp + "/Conv_gate", h, 3, 1) + onp.conv1x1(p, rp + "/gate_conv_c", c)
    o = np.tanh(f) * onp.sigmoid(g)
    want = onp.res_block(p, rp, h, c, 3, 1)[0].reshape(B * T, 256) * (float(SQRT_HALF_F32) / np.sqrt(0.5))
    Wr = onp.wn_kernel_1d(p, rp + "/res_conv")[0].T                         # [n][k]
    got, terms = ref_res(o.reshape(-1, 256), h.reshape(-1, 256), Wr, p[rp + "/res_conv/bias"])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (np.abs(got) <= terms + 1e-12).all()


@pytest.mark.parametrize("block", [0, 2, 3])
def test_tail_epilogue_reference_equals_the_oracle_flow_in_both_directions(block):
    """The oracle's fp64 WaveNet output, taken back in front of its exp(3 scale) factor and permuted to the (log_s | t)
    plane-channel order of save_z, in place of Z: ref_tail_epilogue gives the planes of onp.flow_forward / onp.flow_reverse
    and logdet (M 2 Ch) to 1e-12."""
    hp, p, fp = tiny_flow(block, 11 + block)
    ch, B, T = 1 << block, 2, 5
    M = B * T
    rng = np.random.default_rng(block)
    x = rng.standard_normal((B, T, 2 * ch))
    c = rng.random((B, T, hp.num_mels << (block + 1)))
    br = packing.bitrev_table(block).astype(np.int64)
    cols = np.concatenate([br, ch + br])
    an = an_table64(p, fp, block)
    e3 = np.exp(3.0 * p[fp + "/WaveNet/ZeroConv1d/scale"].reshape(-1))
    ez = e3[cols].reshape(2, ch)

    # forward: the network sees the ActNorm output of in_a
    y = onp.actnorm_forward(p, fp + "/ActNorm", x)[0]
    net = onp.wavenet(p, fp + "/WaveNet", y[:, :, :ch], c[:, :, :c.shape[2] // 2], hp.n_layer)
    Z = (net.reshape(M, 2 * ch) / e3)[:, cols]
    xa, xb = plane_order(x, block)
    r = ref_tail_epilogue(Z, ez, an, xa, xb, 0)
    out, _, logdet = onp.flow_forward(p, fp, x, c, hp)                  # change_order: (out_b | in_a)
    wb, wa = plane_order(out, block)
    assert np.abs(r["oa"] - wa).max() <= 1e-12 and np.abs(r["ob"] - wb).max() <= 1e-12 * max(1.0, np.abs(wb).max())
    assert abs(r["logdet_sum"] - logdet * (M * 2 * ch)) <= 1e-12 * max(1.0, r["logdet_abs"])
    assert np.abs(r["ls"]).max() > 0.3

    # inverse: flow_reverse swaps the halves first, the network sees out_a as it is
    yo, co = onp.change_order(x, c)
    net = onp.wavenet(p, fp + "/WaveNet", yo[:, :, :ch], co[:, :, :c.shape[2] // 2], hp.n_layer)
    Z = (net.reshape(M, 2 * ch) / e3)[:, cols]
    xa, xb = plane_order(yo, block)
    r = ref_tail_epilogue(Z, ez, an, xa, xb, 1)
    back = onp.flow_reverse(p, fp, x, c, hp)[0]
    wa, wb = plane_order(back, block)
    assert np.abs(r["oa"] - wa).max() <= 1e-12 * max(1.0, np.abs(wa).max())
    assert np.abs(r["ob"] - wb).max() <= 1e-12 * max(1.0, np.abs(wb).max())
    # and the two directions invert one another
    rt = onp.flow_reverse(p, fp, out, onp.flow_forward(p, fp, x, c, hp)[1], hp)[0]
    assert np.abs(rt - x).max() <= 1e-10


def test_ez_planes_reads_the_pair_tile_layout():
    for ch in (1, 8, 32, 64, 128):
        npt = npt_of(ch)
        ezero = np.arange(npt * 64, dtype=np.float64)
        got = ez_planes(ezero, ch)
        for tau in range(ch):
            assert got[0, tau] == (tau // 32) * 64 + tau % 32 and got[1, tau] == got[0, tau] + 32


# ------------------------------------------------------------------ the row counts and forms of the GPU cases
def test_res_row_counts_follow_from_the_rule():
    """The row counts derived from the restated rule are the ones the issue's table names: each form's first M has a one-row
    last tile, the second is an exact multiple of the tile height."""
    rc = res_row_counts()
    assert rc == {"splitk64x64": [1, 63, 64, 65, 6080], "64x128": [6081, 6144], "128x128d3": [12161, 12288],
                  "128x128d2": [24321, 24576]}
    for form, ms in rc.items():
        assert all(res_form(m) == form for m in ms)
        if form != "splitk64x64":
            assert res_form(ms[0] - 1) != form and ms[0] % RES_TILE_ROWS[form] == 1 and ms[1] % RES_TILE_ROWS[form] == 0
    assert all(res_form(m) != "256x128" for m in range(1, 70000, 7))


def test_front_forms_and_their_thresholds():
    assert [front_form(ch, False, 300) for ch in (1, 2, 4, 8, 16)] == ["valu_k6_r16", "valu_k6_r16", "valu_k12_r16", "valu_k24_r16", "valu_k48_r16"]
    assert front_form(8, False, 32767) == "valu_k24_r16" and front_form(8, False, 32768) == "valu_k24_r64"
    assert front_form(16, False, 32768) == "valu_k48_r64" and front_form(16, True, 32768) == "mfma16"
    assert [front_form(ch, True, 300) for ch in (16, 32, 64, 128)] == ["mfma16", "mfma32", "mfma64", "mfma128"]
    first = first_rows(lambda m: front_form(32, False, m), hi=40000)
    assert first == {"gemm128_1": 1, "gemm128_2": 255 * 128 + 1}


def test_tail_cases_name_their_forms_and_the_table_is_complete():
    for form, m, ch, stream in TAIL_CASES:
        assert tail_form(m, 2, ch, npt_of(ch), stream and npt_of(ch) == 1)[0] == form, (form, m, ch, stream)
    kinds = {(f, npt_of(ch)) for f, _, ch, _ in TAIL_CASES}
    assert {(f, n) for f in ("split3", "split_chain", "fused128", "fused256") for n in (1, 2, 4)} <= kinds
    assert {("rs1", 1), ("rs2", 1), ("rs4", 1)} <= kinds
    # each form's first row count, from the rule
    assert first_rows(lambda m: tail_form(m, 2, 64, 2, False)[0]) == {"split3": 1, "split_chain": 6144, "fused128": 12289, "fused256": 49152}
    assert first_rows(lambda m: tail_form(m, 2, 8, 1, True)[0]) == {"split3": 1, "rs1": 1008, "rs2": 6144, "rs4": 12288, "fused256": 49152}


def test_tail_form_agrees_with_the_library_queries(lib):
    """fwn_tail_partials_desc(.., -1), fwn_tail_can_chain and fwn_tail_partials against the restated rule, over the case table
    and either side of every threshold, with and without the fragment stream (host code: no GPU)."""
    from test_host import _tail_desc
    ms = sorted({m for _, m, _, _ in TAIL_CASES} | {b + o for b in (64, TRS_MIN_ROWS, TAIL_SPLIT_CHAIN_MIN, TAIL_SPLIT_MAX, TAIL256_MIN)
                                                      for o in (-1, 0, 1)})
    for ch in (1, 8, 16, 32, 64, 128):
        npt = npt_of(ch)
        for stream in (False, True):
            if stream and npt != 1:
                continue
            dp, _ = _tail_desc(ch, 2, npt, stream)
            for m in ms:
                kind, rows = tail_form(m, 2, ch, npt, stream)
                assert lib.fwn_tail_partials_desc(dp, m, -1) == tail_slots(m, 2, ch, npt, stream), (ch, stream, m)
                assert bool(lib.fwn_tail_can_chain(dp, m, 0)) == (kind != "split3"), (ch, stream, m)
                assert bool(lib.fwn_tail_can_chain(dp, m, 1)) == (kind != "split3" and ch <= 8 and npt == 1), (ch, stream, m)
                assert lib.fwn_tail_partials(m) == tail_partials_bound(m) >= tail_slots(m, 2, ch, npt, stream), (ch, stream, m)
