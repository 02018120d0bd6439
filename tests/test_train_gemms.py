"""The GEMMs of a training step - fwn_gemm in every tile and epilogue form, fwn_tn_gemm / fwn_tn_gemm_group,
fwn_transpose_shift, fwn_reduce_splits, fwn_wn_backward_group, fwn_colsum_bf16 - through the C ABI against the plain NumPy
fp64 references of tests/test_train_gemm_refs.py (proved there on the CPU).  Two kinds of case:

(a) exact: small integers stored in bf16 (x in {-2 .. 2}, sparse; w in {-1, 0, 1}; integer bias, R, Y0; power-of-two
    scales).  Every partial sum is an integer below 2^24, exact in fp32 in any order, so the kernel must equal the
    reference BIT FOR BIT - a wrong index, tap, chunk tail, split boundary or tile edge shows whatever its size.  For
    bf16 outputs the reference itself is asserted to stay within +-256 (integers a bf16 holds exactly).
(b) bounded: random normal operands against per-element bounds.  None is fitted; with u = 2^-24 and the factor 2 as
    head-room for u^2 (as in test_train_stages.py):
    fwn_gemm, fp32 output:  |got - want| <= 2 (K + 4) u |oscale| (sum |x w| + |bias| + |rscale R|) + 2 u (|Y0| + |want|),
                            K = sum_s k_s: one fp32 rounding per accumulated product in any order, plus the epilogue's few
                            operations; bf16 output: the same plus 2^-8 |want| (the cast: half an ulp of 8 bits).
    fwn_tn_gemm partial z:  <= 2 (rows_z + 1) u sum_{m in z} |x dy|; the bias row the same with sum |dy|.
    fwn_reduce_splits, db, dV without weight norm: <= 2 (nsplit + 2) u |scale| sum_s |part_s| =: delta (nsplit - 1 adds,
                            the scale, the store).
    dg, dV with weight norm: the kernel keeps dW in fp32 (within delta of the exact one) and does everything after it in
                            fp64 with ONE cast at the end, so delta goes through the formulas linearly:
                            e_g = sum_k delta[k] |V[k]| / nrm,  |dg - want| <= e_g + 2 u |dg|,
                            |dV - want| <= (|g| / nrm) (delta + |V| e_g / nrm) + 2 u |dV|.
    fwn_colsum_bf16:        colsum_bf16_kernel gives each of its nb = fwn_colsum_partials / C row blocks (per = ceil(M / nb)
                            rows) to four thread groups; a group adds its p <= ceil(per / 4) bf16 values (exact in fp32) in
                            fp32: p - 1 roundings; the four are added as a tree: 2 more on any path; the partial is
                            stored as that fp32.  colsum_final_kernel adds the partials and applies the scale in fp64
                            and casts once: 1 more.  Each rounding is at most u times the sum of the absolute terms
                            below it, so  |got - want| <= 2 (ceil(per / 4) + 2) u |scale| sum_m |dy|.

Every case asserts, through fwn_gemm_tile / fwn_tn_gemm_tile, the tile it is there to reach.  Outputs start as a
sentinel, partials and scratch as NaN, with guards behind every buffer; W columns outside every segment and X columns
[k, ld) hold 1e30 (finite padding is the contract)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tf_flowavenet_amd import _lib

from test_train_stages import GUARD, SENT, U, assert_within, dev, guard_intact, host, same_bits, scratch, stream
from test_train_gemm_refs import (GEMM_TILES, T32, T64, T128, T256, ref_gemm, ref_tn_gemm, ref_wn_backward,
                                  tap_rows, tn_split_rows)

pytestmark = pytest.mark.gpu

BIG = 1e30
RATIOS = {}          # worst err / bound per kernel and form over the bounded cases (printed by the last test)


def note_ratio(key, got, want, bound):
    assert_within(got, want, bound, key)
    err = np.abs(got.astype(np.float64) - want)
    nz = bound > 0
    r = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("err / bound %-28s %.3f" % (key, r))


def to_bf16(a):
    """fp32 values rounded to bf16 (round to nearest even), as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def bdev(a, guard=GUARD):
    """NumPy array of bf16-representable values -> flat bf16 device tensor followed by `guard` sentinel elements."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = torch.full((a.size + guard,), SENT, dtype=torch.bfloat16, device="cuda")
    t[:a.size] = torch.from_numpy(a.reshape(-1)).cuda().to(torch.bfloat16)
    return t


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def padded(a, ld, fill):
    """[M][n] -> [M][ld] with `fill` in the columns [n, ld)."""
    out = np.full((a.shape[0], ld), fill, dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


# =================================================================== fwn_gemm
class GemmProblem:
    """One fwn_gemm problem in NumPy (values exactly representable in the type the kernel reads) and on the device.
    xs: list of (rows, ld, k) source matrices; segs: list of (index into xs, shift).  Segment s lies in W's columns
    [koff_s, koff_s + k) with koff_0 = 8 and 8 columns of 1e30 between segments and behind the last one (ldw > sum k)."""

    def __init__(self, name, seed, xs, segs, Ti=0, exact=True, bias=False, R=False, mask=False, relu=False, rscale=1.0,
                 oscale=1.0, out_f32=False, accumulate=False, nsplit=1):
        self.M, self.N, ns, self.tile = GEMM_TILES[name]
        assert ns == nsplit
        M, N = self.M, self.N
        self.name, self.Ti, self.exact, self.relu, self.out_f32, self.accumulate, self.nsplit = name, Ti, exact, relu, out_f32, accumulate, nsplit
        self.rscale, self.oscale = float(np.float32(rscale)), float(np.float32(oscale))
        rng = np.random.default_rng(seed)
        self.X = []
        for rows, ld, k in xs:
            x = np.full((rows, ld), to_bf16(np.float32(BIG)), dtype=np.float32)
            if exact:
                v = rng.integers(-2, 3, (rows, k)) * (rng.random((rows, k)) < 0.1)
                if Ti > 0:           # the rows next to a clip edge are dense: a tap that crosses the edge changes the result
                    t = np.arange(rows) % Ti
                    edge = (t < 3) | (t >= Ti - 3)
                    v[edge] = rng.choice([-1, 1], (int(edge.sum()), k))
                x[:, :k] = v
            else:
                x[:, :k] = to_bf16(rng.standard_normal((rows, k)) * 0.5)
            self.X.append(x)
        self.segs, koff = [], 8
        for xi, shift in segs:
            k = xs[xi][2]
            self.segs.append((xi, k, shift, koff))
            koff += k + 8
        self.K, self.ldw = sum(s[1] for s in self.segs), koff
        self.W = np.full((N, self.ldw), to_bf16(np.float32(BIG)), dtype=np.float32)
        for xi, k, shift, ko in self.segs:
            self.W[:, ko:ko + k] = rng.integers(-1, 2, (N, k)) if exact else to_bf16(rng.standard_normal((N, k)) * 0.05)
        self.bias = self.R = self.mask = self.Y0 = None
        if bias:
            self.bias = (rng.integers(-4, 5, N) if exact else rng.standard_normal(N)).astype(np.float32)
        if R:
            self.R = rng.integers(-8, 9, (M, N)).astype(np.float32) if exact else to_bf16(rng.standard_normal((M, N)))
        if mask:
            self.mask = to_bf16(rng.standard_normal((M, N)))
            z = rng.random((M, N))
            self.mask[z < 0.1] = 0.0
            self.mask[z > 0.9] = -0.0
        if accumulate:
            self.Y0 = (rng.integers(-16, 17, (M, N)) if exact else rng.standard_normal((M, N))).astype(np.float32)
        self.d_X = [bdev(x) for x in self.X]
        self.d_W = bdev(self.W)
        self.d_bias = dev(self.bias) if bias else None
        self.keep = []

    def reference(self, row_len=None, len_spr=1, segs=None):
        segs = [(self.X[xi], k, sh, ko) for xi, k, sh, ko in self.segs] if segs is None else segs
        y, terms = ref_gemm(segs, self.W, self.M, self.N, self.Ti, self.bias, self.R, self.rscale, self.mask, self.relu, self.oscale,
                            self.Y0, row_len, len_spr, with_abs=not self.exact)
        if self.exact:
            assert np.abs(y).max() < 2.0 ** 24 and (self.out_f32 or np.abs(y).max() <= 256.0), np.abs(y).max()
            assert (y * 2 == np.round(y * 2)).all()
        return y, terms

    def bound(self, want, terms):
        b = 2.0 * (self.K + 4) * U * terms + 2.0 * U * ((np.abs(self.Y0) if self.Y0 is not None else 0.0) + np.abs(want))
        return b if self.out_f32 else b + 2.0 ** -8 * np.abs(want)

    def launch(self, ldy=None, ldr=None, ldmask=None, row_len=None, len_spr=1, gate=None, split_stride=None):
        """Runs fwn_gemm; returns Y [M][N] (nsplit > 1: [nsplit][M][N]) as fp32 NumPy after checking that the columns
        [N, ldy), the gap behind every split and the guards behind every buffer still hold the sentinel."""
        lib = _lib.load()
        M, N = self.M, self.N
        ldy, ldr, ldmask = ldy or N, ldr or N, ldmask or N
        d = _lib.GemmDesc()
        for i, (xi, k, shift, ko) in enumerate(self.segs):
            s = d.seg[i]
            s.x, s.rows, s.ld, s.k, s.shift, s.koff = self.d_X[xi].data_ptr(), self.X[xi].shape[0], self.X[xi].shape[1], k, shift, ko
        d.nseg, d.M, d.N, d.Ti = len(self.segs), M, N, self.Ti
        d.W, d.ldw = self.d_W.data_ptr(), self.ldw
        d.bias = self.d_bias.data_ptr() if self.d_bias is not None else None
        bufs = []
        if self.R is not None:
            d_R = bdev(padded(self.R, ldr, SENT))
            d.R, d.ldr, d.rscale = d_R.data_ptr(), ldr, self.rscale
            bufs.append((d_R, M * ldr))
        if self.mask is not None:
            d_m = bdev(padded(self.mask, ldmask, SENT))
            d.mask, d.ldmask = d_m.data_ptr(), ldmask
            bufs.append((d_m, M * ldmask))
        stride = split_stride or M * ldy
        y0 = np.full((self.nsplit, stride), SENT, dtype=np.float32)
        body = y0[:, :M * ldy].reshape(self.nsplit, M, ldy)
        if self.Y0 is not None:
            body[:, :, :N] = self.Y0
        elif self.nsplit > 1:
            body[:, :, :N] = np.nan              # partials: every one must come back fully written
        d_Y = dev(y0) if self.out_f32 else bdev(y0)
        d.Y, d.ldy, d.out_f32, d.accumulate, d.nsplit, d.split_stride = d_Y.data_ptr(), ldy, int(self.out_f32), int(self.accumulate), self.nsplit, stride
        d.relu, d.oscale = int(self.relu), self.oscale
        if gate is not None:
            d.gate_aux, d.gate_out, d.gate_col0 = gate[0].data_ptr(), gate[1].data_ptr(), gate[2]
        if row_len is not None:
            d_len = dev(np.asarray(row_len, np.int32), 0)
            d.row_len, d.len_spr = d_len.data_ptr(), len_spr
        assert lib.fwn_gemm_tile(C.byref(d)) == self.tile, (self.name, lib.fwn_gemm_tile(C.byref(d)))
        _lib.check(lib.fwn_gemm(C.byref(d), stream()), "fwn_gemm")
        torch.cuda.synchronize()
        assert guard_intact(d_Y, self.nsplit * stride) and all(guard_intact(t, n) for t, n in bufs)
        got = d_Y[:self.nsplit * stride].float().cpu().numpy().reshape(self.nsplit, stride)
        assert (got[:, M * ldy:] == SENT).all()
        got = got[:, :M * ldy].reshape(self.nsplit, M, ldy)
        assert (got[:, :, N:] == SENT).all(), "columns [N, ldy) were written"
        return got[:, :, :N].copy() if self.nsplit > 1 else got[0, :, :N].copy()

    def inputs_intact(self):
        ok = all(guard_intact(t, x.size) and np.array_equal(t[:x.size].float().cpu().numpy().reshape(x.shape), x) for t, x in zip(self.d_X, self.X))
        return ok and guard_intact(self.d_W, self.W.size) and np.array_equal(self.d_W[:self.W.size].float().cpu().numpy().reshape(self.W.shape), self.W)


def clip_len(M, cands):
    """The first candidate clip length that divides M (0: no clips)."""
    for t in cands:
        if t and M % t == 0:
            return t
    return 0


def check(p, got, want, terms, key):
    if p.exact:
        bad = bits32(got) != bits32(want + 0.0)      # + 0.0: the epilogue ends in `+ Y0 | + 0`, which never leaves a -0
        assert not bad.any(), "%s: %d of %d elements differ from the exact result, first at %s" % (
            key, int(bad.sum()), bad.size, np.unravel_index(np.argmax(bad), bad.shape))
    else:
        note_ratio(key, got, want, p.bound(want, terms))


# ---- the tile x epilogue grid: every big tile in the row-major AND the direct epilogue, the 32 x 64 tile (always direct)
GRID = [("t32_a", (40,)), ("t32_n4", (0,)), ("t32_row", (0,)), ("t64", (325,)), ("t128", (175,)), ("t256", (0,)), ("t256_tail1", (197,))]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32acc"])
@pytest.mark.parametrize("name,ti", GRID)
def test_gemm_every_tile_in_both_epilogue_forms(name, ti, out_f32, exact):
    """Three taps of a k = 72 matrix (ld 80) with clip edges (or, Ti == 0, the bounds of a matrix of M + 2 rows) and a k = 8
    segment, bias + rscale R + mask + relu + oscale, bf16 output or fp32 accumulate.  The same problem with ldy = N (N % 8 == 0:
    the row-major epilogue of the big tiles), ldy = N + 2, ldr = N + 2 and ldmask = N + 6 (each alone sends the launch to
    the direct epilogue): equal bit for bit, as the comment above LDS_EPI claims, and equal to the reference."""
    M, N, _, tile = GEMM_TILES[name]
    Ti = clip_len(M, ti)
    rows = M if Ti else M + 2
    p = GemmProblem(name, 1, [(rows, 80, 72), (rows, 8, 8)], [(0, -1), (0, 0), (0, 1), (1, 0)], Ti=Ti, exact=exact, bias=True, R=True,
                    mask=True, relu=True, rscale=0.5, oscale=2.0, out_f32=out_f32, accumulate=out_f32)
    want, terms = p.reference()
    layouts = [dict(ldy=N + 2), dict(ldr=N + 2), dict(ldmask=N + 6)]
    if N % 8 == 0:
        layouts.insert(0, dict())
    first = None
    for lay in layouts:
        got = p.launch(**lay)
        check(p, got, want, terms, "gemm %d %s %s" % (tile, "f32" if out_f32 else "bf16", "rows" if not lay and tile != T32 else "direct"))
        first = got if first is None else first
        assert same_bits(got, first), "layout %r changes the bits" % (lay,)
    assert same_bits(p.launch(**layouts[0]), first)           # a repeat
    assert p.inputs_intact()


# ---- the front-conv data gradient as production runs it: N = Ch, ldy = N, fp32 accumulate, three taps of k = 256
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("name,ti", [("front32", 300), ("front64", 215), ("front128", 1025), ("front256", 1025),
                                     ("front32_n2", 300), ("front64_n4", 215), ("front128_n2", 1025), ("front256_n4", 1025)])
def test_gemm_front_conv_data_gradient_on_every_tile(name, ti, exact):
    """N in {1, 2, 4}: no 8-column group is whole, every tile takes the direct epilogue; clips of Ti rows, Ti a multiple of
    no tile, so clip edges fall inside row tiles and wave tiles."""
    M, N, _, tile = GEMM_TILES[name]
    assert M % ti == 0 and all(ti % e for e in (32, 64, 128, 256))
    p = GemmProblem(name, 2, [(M, 256, 256)], [(0, 1), (0, 0), (0, -1)], Ti=ti, exact=exact, out_f32=True, accumulate=True)
    want, terms = p.reference()
    got = p.launch()
    check(p, got, want, terms, "gemm %d front N<8" % tile)
    assert same_bits(p.launch(), got) and p.inputs_intact()


# ---- K edges: a segment below one chunk, one that ends inside a chunk, one that crosses a 128 chunk; mixed ld / rows
KCASES = {
    "k8": ([(0, 8, 8)], [(0, 0)]),
    "k72": ([(0, 80, 72)], [(0, 0)]),
    "k136": ([(0, 136, 136)], [(0, 0)]),
    "mixed": ([(5, 80, 72), (0, 144, 136), (1, 8, 8)], [(0, 2), (1, 0), (2, -1)]),      # (extra rows, ld, k), (matrix, shift); Ti == 0
}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("kcase", sorted(KCASES))
@pytest.mark.parametrize("name", ["k32", "k128"])
def test_gemm_k_edges(name, kcase, exact):
    """koff = 8 and ldw > sum k with 1e30 around every segment, X padding columns 1e30: the `kk < k` predicates of both
    operands.  k = 8 alone is the ZeroConv data gradient (k = ldz = 8)."""
    M, N, _, tile = GEMM_TILES[name]
    xs, segs = KCASES[kcase]
    p = GemmProblem(name, 3, [(M + extra, ld, k) for extra, ld, k in xs], segs, exact=exact, bias=True)
    want, terms = p.reference()
    for lay in (dict(), dict(ldy=N + 2)):
        check(p, p.launch(**lay), want, terms, "gemm %d K edge" % tile)
    assert p.inputs_intact()


@pytest.mark.parametrize("name,ti", [("bounds32", 50), ("bounds64", 200)])
def test_gemm_matrix_bounds_and_a_tap_that_is_zero_everywhere(name, ti):
    """Ti == 0: only the bounds of each segment's own matrix apply - one has fewer rows than M (its tail reads zero), one
    more.  Ti > 0 with shifts -Ti and Ti + 7: both outer taps are zero in every row.  Exact."""
    M, N, _, tile = GEMM_TILES[name]
    p = GemmProblem(name, 4, [(M - 5, 72, 72), (M + 4, 16, 8)], [(0, 2), (1, -3), (0, -4)], Ti=0)
    want, _ = p.reference()
    assert np.array_equal(want[M - 7:], ref_gemm([(p.X[1], 8, -3, p.segs[1][3]), (p.X[0], 72, -4, p.segs[2][3])], p.W, M, N, with_abs=False)[0][M - 7:])
    check(p, p.launch(), want, None, "bounds")
    check(p, p.launch(ldy=N + 2), want, None, "bounds")
    q = GemmProblem(name, 5, [(M, 72, 72)], [(0, -ti), (0, 0), (0, ti + 7)], Ti=ti)
    want, _ = q.reference()
    assert np.array_equal(want, ref_gemm([(q.X[0], 72, 0, q.segs[1][3])], q.W, M, N, with_abs=False)[0])
    check(q, q.launch(), want, None, "zero taps")
    check(q, q.launch(ldy=N + 2), want, None, "zero taps")
    assert p.inputs_intact() and q.inputs_intact()


# ---- epilogue operands, singly and together
@pytest.mark.parametrize("name,ti", [("epi32", 40), ("epi64", 325), ("epi256", 0)])
def test_gemm_epilogue_operands_singly_and_together(name, ti):
    """bias | rscale R | mask (+0 and -0 drop) | relu | oscale alone and all together, each as a bf16 store, an fp32 store and
    an fp32 accumulate; exact for every combination, and the all-together one also with random operands against the bound."""
    M, N, _, tile = GEMM_TILES[name]
    combos = [dict(bias=True), dict(R=True, rscale=0.5), dict(R=True, rscale=-2.0), dict(mask=True), dict(relu=True), dict(oscale=-0.5),
              dict(bias=True, R=True, rscale=0.5, mask=True, relu=True, oscale=2.0)]
    for c in combos:
        for out_f32, acc in ((False, False), (True, False), (True, True)):
            p = GemmProblem(name, 6, [(M, 16, 8), (M, 8, 8)], [(0, -1), (0, 1), (1, 0)], Ti=ti, out_f32=out_f32, accumulate=acc, **c)
            want, _ = p.reference()
            got = p.launch()
            check(p, got, want, None, "epilogue %r" % (c,))
            if acc:
                check(p, p.launch(ldy=N + 2), want, None, "epilogue %r direct" % (c,))
    for out_f32 in (False, True):
        p = GemmProblem(name, 7, [(M, 72, 72), (M, 8, 8)], [(0, -1), (0, 1), (1, 0)], Ti=ti, exact=False, out_f32=out_f32, accumulate=out_f32, **combos[-1])
        want, terms = p.reference()
        check(p, p.launch(), want, terms, "gemm %d %s all operands" % (tile, "f32" if out_f32 else "bf16"))
        check(p, p.launch(ldr=N + 2), want, terms, "gemm %d %s all operands direct" % (tile, "f32" if out_f32 else "bf16"))


# ---- split-K
def split_segments(p):
    """The segments of every split: chunks of BK columns (128 on the 32 x 64 and 64 x 128 tiles, 64 on the others) in segment
    order, per = ceil(chunks / nsplit) chunks per split, as `lin_kernel` deals them."""
    bk = 128 if p.tile in (T32, T64) else 64
    chunks = [(xi, min(bk, k - c), sh, ko, c) for xi, k, sh, ko in p.segs for c in range(0, k, bk)]
    per = (len(chunks) + p.nsplit - 1) // p.nsplit
    return [[(p.X[xi][:, c:], kk, sh, ko + c) for xi, kk, sh, ko, c in chunks[z * per:(z + 1) * per]] for z in range(p.nsplit)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("name,ti,ks,empty", [("split32_2", 100, (136, 72), 0), ("split64_4", 175, (136, 72, 8, 136), 1),
                                              ("split128_over", 525, (136,), 1), ("split256_4", 525, (136, 72, 136), 0)])
def test_gemm_split_k_partials_and_their_reduction(name, ti, ks, empty, exact):
    """nsplit in {2, 4}; split128_over has 3 chunks of 64 for 4 splits.  Every partial comes back fully written (they start as
    NaN), the empty ones as zeros; each equals the reference of its own chunks; split_stride > M ldy leaves the gap alone;
    fwn_reduce_splits (scale != 1, stride > n) adds them within 2 (nsplit + 2) u |scale| sum |part|."""
    lib = _lib.load()
    M, N, nsplit, tile = GEMM_TILES[name]
    p = GemmProblem(name, 8, [(M, k + 8, k) for k in ks], [(i, (-1, 0, 1)[i % 3]) for i in range(len(ks))], Ti=ti, exact=exact, out_f32=True, nsplit=nsplit)
    stride = M * N + 12
    got = p.launch(split_stride=stride)
    assert not np.isnan(got).any()
    per_split = split_segments(p)
    assert sum(1 for s in per_split if not s) == empty
    total, total_abs = np.zeros((M, N)), np.zeros((M, N))
    for z, segs in enumerate(per_split):
        if not segs:
            assert same_bits(got[z], np.zeros((M, N), np.float32))
            continue
        want, terms = p.reference(segs=segs)
        total, total_abs = total + want, total_abs + np.abs(got[z].astype(np.float64))
        if exact:
            check(p, got[z], want, None, "split %d" % z)
        else:
            kz = sum(s[1] for s in segs)
            note_ratio("gemm %d split partial" % tile, got[z], want, 2.0 * (kz + 4) * U * terms + 2.0 * U * np.abs(want))
    assert same_bits(p.launch(split_stride=stride), got)
    scale = 0.25 if exact else float(np.float32(-1.7))
    d_part = dev(padded(got.reshape(nsplit, M * N), stride, SENT))
    out = scratch(M * N)
    _lib.check(lib.fwn_reduce_splits(d_part.data_ptr(), nsplit, stride, M * N, scale, out.data_ptr(), stream()), "fwn_reduce_splits")
    torch.cuda.synchronize()
    assert guard_intact(out, M * N) and guard_intact(d_part, nsplit * stride)
    red = host(out, (M, N))
    if exact:
        assert same_bits(red, (scale * total).astype(np.float32))
    else:
        note_ratio("reduce_splits", red, scale * got.astype(np.float64).sum(0), 2.0 * (nsplit + 2) * U * abs(scale) * total_abs)
    assert p.inputs_intact()


@pytest.mark.parametrize("nsplit,n", [(1, 1000), (2, 1000), (7, 1000), (7, 2048 * 256 + 77)])
def test_reduce_splits_alone(nsplit, n):
    """nsplit in {1, 2, 7}, stride > n, scale != 1; the last size is past one pass of the capped grid."""
    lib = _lib.load()
    rng = np.random.default_rng(nsplit + n)
    stride, scale = n + 3, float(np.float32(0.3))
    part = rng.standard_normal((nsplit, n)).astype(np.float32)
    d_part, out = dev(padded(part, stride, BIG)), scratch(n)
    res = []
    for rep in range(2):
        _lib.check(lib.fwn_reduce_splits(d_part.data_ptr(), nsplit, stride, n, scale, out.data_ptr(), stream()), "fwn_reduce_splits")
        torch.cuda.synchronize()
        res.append(host(out, (n,)).copy())
    p64 = part.astype(np.float64)
    note_ratio("reduce_splits", res[0], scale * p64.sum(0), 2.0 * (nsplit + 2) * U * abs(scale) * np.abs(p64).sum(0))
    assert same_bits(res[0], res[1]) and guard_intact(out, n) and guard_intact(d_part, nsplit * stride)
    assert same_bits(host(d_part, (nsplit, stride)), padded(part, stride, BIG))


# ---- row lengths
@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("name,ti", [("rl32", 24), ("rl64", 200), ("rl128", 1025), ("rl256", 1025)])
def test_gemm_row_lengths_zero_the_rows_past_each_clip_and_nothing_else(name, ti, out_f32):
    """row_len on every tile in both epilogues: clips of full length, one row, no row, more than full, and lengths that are no
    multiple of len_spr = 2 (len // 2 rows).  Rows past an end are exact zeros although the product there is not (the
    operands are dense near the clip edges); every other row has the bits of the call without lengths, which itself equals
    the exact reference."""
    M, N, _, tile = GEMM_TILES[name]
    nclip = M // ti
    lens = np.array(([2 * ti, 3, 0, 2 * (ti // 2) + 1, 2, 2 * ti + 5, 2 * ti - 1, 1] * nclip)[:nclip], np.int32)
    p = GemmProblem(name, 9, [(M, 72, 72)], [(0, -1), (0, 0), (0, 1)], Ti=ti, bias=True, R=True, rscale=0.5, oscale=2.0, out_f32=out_f32)
    want, _ = p.reference()
    want_len, _ = p.reference(row_len=lens, len_spr=2)
    pad = (np.arange(M) % ti) >= (lens[np.arange(M) // ti] // 2)
    assert pad.any() and (~pad).any() and np.abs(want[pad]).min(1).max() > 0
    for lay in (dict(), dict(ldy=N + 2)):
        plain, ragged = p.launch(**lay), p.launch(row_len=lens, len_spr=2, **lay)
        check(p, plain, want, None, "plain")
        check(p, ragged, want_len, None, "row_len")
        assert same_bits(ragged[pad], np.zeros_like(ragged[pad])) and same_bits(ragged[~pad], plain[~pad])
    assert p.inputs_intact()


# ---- the gate derivative
@pytest.mark.parametrize("name,ti", [("gate32", 100), ("gate64", 125), ("gate128", 175), ("gate256", 275)])
def test_gemm_gate_derivative_on_every_tile_epilogue_and_column_block(name, ti):
    """gate_aux: the 256 columns from gate_col0 in {0, 256, 512} of N = 768 leave through the gate's derivative - bit for bit
    what storing them and running fwn_gate_bwd gives (that kernel has its own fp64 test in test_train_stages.py) - in both
    epilogues (ldy = N and N + 2), without and with row_len.  The ungated columns have the plain call's bits, the gated
    columns of Y stay untouched, eight rows behind gate_out too."""
    lib = _lib.load()
    M, N, _, tile = GEMM_TILES[name]
    assert N == 768 and M % ti == 0
    rng = np.random.default_rng(10)
    p = GemmProblem(name, 10, [(M, 256, 256)], [(0, 0)], Ti=ti, exact=False, R=True, rscale=0.5, oscale=0.7)
    aux = bdev(np.concatenate([np.tanh(rng.standard_normal((M, 256))), 1 / (1 + np.exp(-rng.standard_normal((M, 256))))], 1), guard=8 * 512)
    nclip = M // ti
    lens = np.array(([2 * ti, 2, 0, 2 * ti - 3] * nclip)[:nclip], np.int32)
    pad = (np.arange(M) % ti) >= (lens[np.arange(M) // ti] // 2)
    for ldy in (N, N + 2):
        for rl in (None, lens):
            kw = dict(ldy=ldy) if rl is None else dict(ldy=ldy, row_len=rl, len_spr=2)
            plain = p.launch(**kw)
            d_plain = bdev(padded(plain, ldy, SENT))
            for col0 in (0, 256, 512):
                want = torch.full((M * 512 + 8 * 512,), SENT, dtype=torch.bfloat16, device="cuda")
                _lib.check(lib.fwn_gate_bwd(d_plain.data_ptr() + 2 * col0, ldy, aux.data_ptr(), M, want.data_ptr(), stream()), "fwn_gate_bwd")
                dpre = torch.full((M * 512 + 8 * 512,), SENT, dtype=torch.bfloat16, device="cuda")
                dpre[:M * 512] = float("nan")
                got = p.launch(gate=(aux, dpre, col0), **kw)
                torch.cuda.synchronize()
                assert torch.equal(bits(dpre), bits(want)), (ldy, col0, rl is not None)
                gated = np.zeros(N, bool)
                gated[col0:col0 + 256] = True
                assert (got[:, gated] == SENT).all() and same_bits(got[:, ~gated], plain[:, ~gated])
                if rl is not None:
                    assert bool((dpre[:M * 512].view(M, 512)[torch.from_numpy(pad).cuda()] == 0).all())
    assert p.inputs_intact() and bool((aux[M * 512:] == SENT).all())


# =================================================================== fwn_tn_gemm
# (The `col < Kx` / `col < N` tests of the kernel's operand loads cannot show in any output: a column of x is an output ROW
# of the product, and rows kx >= Kx - like columns >= N - are dropped by the store predicate.  The 1e30 padding behind
# Kx and around dy is there for the store side: a row or column too many would carry it into a partial.)
def tn_problem(seed, M, Kx, N, exact, Ti):
    """x [M][Kx + 8] (padding 1e30), dy = columns [8, 8 + N) of a [M][N + 16] matrix whose other columns are 1e30."""
    rng = np.random.default_rng(seed)
    x, wide = np.full((M, Kx + 8), to_bf16(np.float32(BIG)), np.float32), np.full((M, N + 16), to_bf16(np.float32(BIG)), np.float32)
    if exact:
        v = rng.integers(-2, 3, (M, Kx)) * (rng.random((M, Kx)) < 0.3)
        if Ti > 0:
            t = np.arange(M) % Ti
            edge = (t < 3) | (t >= Ti - 3)
            v[edge] = rng.choice([-2, -1, 1, 2], (int(edge.sum()), Kx))
        x[:, :Kx], wide[:, 8:8 + N] = v, rng.integers(-1, 2, (M, N))
    else:
        x[:, :Kx], wide[:, 8:8 + N] = to_bf16(rng.standard_normal((M, Kx)) * 0.5), to_bf16(rng.standard_normal((M, N)) * 0.1)
    return x, wide


def tn_buffer(nsplit, size, stride):
    """[nsplit][stride] fp32: NaN where a partial goes, the sentinel in the gap behind each, then the guard."""
    t = scratch(nsplit * stride)
    t[:nsplit * stride].view(nsplit, stride)[:, size:] = SENT
    return t


# (M, Ti, Kx, N, ntap, shift0, dshift, nsplit, bias_row, tile)
TN_CASES = [
    (1, 0, 8, 8, 1, 0, 0, 1, 1, 128),
    (63, 21, 80, 72, 3, -1, 1, 1, 0, 128),
    (65, 0, 136, 256, 1, 0, 0, 5, 1, 128),         # 2 chunks for 5 splits: per = 1, three empty
    (127, 0, 264, 264, 1, 0, 0, 3, 1, 128),        # three 128-wide row and column tiles, the last 8 wide; one empty split
    (128, 0, 640, 8, 1, 0, 0, 1, 0, 256),
    (129, 43, 8, 264, 3, -43, 43, 3, 1, 256),      # dshift = Ti: taps 0 and 2 are zero everywhere; Kx = 8 (front conv of blocks 0 - 3)
    (333, 111, 264, 72, 3, -3, 3, 3, 1, 256),      # Ti no multiple of 64: clip edges inside chunks and across split boundaries
    (333, 111, 80, 256, 3, -1, 1, 1, 1, 256),
    (333, 0, 136, 264, 3, -2, 2, 3, 0, 256),       # Ti == 0: the matrix bounds
]


def run_tn(lib, d_x, ldx, Kx, ntap, shift0, dshift, dy_ptr, ldy, N, M, Ti, nsplit, bias_row):
    size = (ntap * Kx + (1 if bias_row else 0)) * N
    stride = size + 5
    part = tn_buffer(nsplit, size, stride)
    _lib.check(lib.fwn_tn_gemm(d_x.data_ptr(), ldx, Kx, ntap, shift0, dshift, dy_ptr, ldy, N, M, Ti, nsplit, part.data_ptr(), stride,
                               bias_row, stream()), "fwn_tn_gemm")
    torch.cuda.synchronize()
    assert guard_intact(part, nsplit * stride)
    got = host(part, (nsplit, stride))
    assert (got[:, size:] == SENT).all() and not np.isnan(got[:, :size]).any()
    return got[:, :size].reshape(nsplit, size // N, N).copy()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("M,Ti,Kx,N,ntap,shift0,dshift,nsplit,bias_row,tile", TN_CASES)
def test_tn_gemm_partials(M, Ti, Kx, N, ntap, shift0, dshift, nsplit, bias_row, tile, exact):
    """Both tiles, ldx > Kx, dy a 16-byte-aligned column block of a wider matrix, taps with clip edges, splits including
    empty ones (zeros), the bias row on and off; partials [nsplit][stride > size] start as NaN."""
    lib = _lib.load()
    assert lib.fwn_tn_gemm_tile(M) == tile
    x, wide = tn_problem(M * 7 + Kx, M, Kx, N, exact, Ti)
    d_x, d_dy = bdev(x), bdev(wide)
    want, wabs, rows = ref_tn_gemm(x, wide[:, 8:], M, Kx, N, ntap, shift0, dshift, Ti, nsplit, bool(bias_row))
    args = (lib, d_x, Kx + 8, Kx, ntap, shift0, dshift, d_dy.data_ptr() + 16, N + 16, N, M, Ti, nsplit, bias_row)
    got = run_tn(*args)
    for z in range(nsplit):
        if rows[z] == 0:
            assert same_bits(got[z], np.zeros_like(got[z])), "empty split %d" % z
    if exact:
        assert np.abs(want).max() < 2.0 ** 24
        bad = bits32(got) != bits32(want)
        assert not bad.any(), "%d elements differ, first at %s" % (int(bad.sum()), np.unravel_index(np.argmax(bad), bad.shape))
    else:
        bound = 2.0 * (np.array(rows, np.float64)[:, None, None] + 1) * U * wabs
        R = ntap * Kx
        note_ratio("tn_gemm %d" % tile, got[:, :R], want[:, :R], bound[:, :R])
        if bias_row:
            note_ratio("tn_gemm %d bias row" % tile, got[:, R:], want[:, R:], bound[:, R:])
    assert same_bits(run_tn(*args), got)
    assert guard_intact(d_x, x.size) and guard_intact(d_dy, wide.size)
    assert np.array_equal(d_x[:x.size].float().cpu().numpy().reshape(x.shape), x) and np.array_equal(d_dy[:wide.size].float().cpu().numpy().reshape(wide.shape), wide)


@pytest.mark.parametrize("M,Ti,tile", [(100, 50, 128), (333, 111, 256)])
def test_tn_gemm_group_equals_each_job_alone(M, Ti, tile):
    """Six jobs of different (Kx, N, ntap, nsplit, bias_row) in one launch: each partial equal bit for bit to the same job through
    fwn_tn_gemm, and (exact operands) to the reference."""
    lib = _lib.load()
    assert lib.fwn_tn_gemm_tile(M) == tile
    specs = [(8, 264, 3, 1, 1), (264, 8, 1, 3, 1), (136, 72, 3, 2, 0), (80, 256, 1, 7, 1), (640, 72, 1, 1, 1), (72, 136, 3, 3, 1)]
    arr = (_lib.TnJob * len(specs))()
    keep, alone = [], []
    for i, (q, (Kx, N, ntap, nsplit, bias_row)) in enumerate(zip(arr, specs)):
        x, wide = tn_problem(i + M, M, Kx, N, True, Ti)
        d_x, d_dy = bdev(x), bdev(wide)
        size = (ntap * Kx + bias_row) * N
        part = tn_buffer(nsplit, size, size + 5)
        keep.append((d_x, d_dy, part, size, x, wide))
        q.x, q.dy, q.part, q.split_stride = d_x.data_ptr(), d_dy.data_ptr() + 16, part.data_ptr(), size + 5
        q.ldx, q.Kx, q.ntap, q.shift0, q.dshift, q.ldy, q.N, q.nsplit, q.bias_row = Kx + 8, Kx, ntap, -2 if ntap == 3 else 0, 2 if ntap == 3 else 0, N + 16, N, nsplit, bias_row
        alone.append(run_tn(lib, d_x, Kx + 8, Kx, ntap, q.shift0, q.dshift, d_dy.data_ptr() + 16, N + 16, N, M, Ti, nsplit, bias_row))
    _lib.check(lib.fwn_tn_gemm_group(arr, len(specs), M, Ti, stream()), "fwn_tn_gemm_group")
    torch.cuda.synchronize()
    for (Kx, N, ntap, nsplit, bias_row), (d_x, d_dy, part, size, x, wide), one, q in zip(specs, keep, alone, arr):
        assert guard_intact(part, nsplit * (size + 5))
        got = host(part, (nsplit, size + 5))
        assert (got[:, size:] == SENT).all()
        got = got[:, :size].reshape(one.shape)
        assert same_bits(got, one)
        want, _, _ = ref_tn_gemm(x, wide[:, 8:], M, Kx, N, ntap, q.shift0, q.dshift, Ti, nsplit, bool(bias_row))
        assert not (bits32(got) != bits32(want)).any()


# =================================================================== fwn_transpose_shift
@pytest.mark.parametrize("ones_row", [0, 1])
@pytest.mark.parametrize("M,C_,ld_src,ld_dst,ntap,shift0,dshift,Ti", [(150, 72, 80, 160, 3, -2, 2, 50), (65, 8, 8, 65, 1, 3, 0, 0),
                                                                     (130, 100, 104, 192, 3, -70, 70, 65)])
def test_transpose_shift_moves_the_right_bits(M, C_, ld_src, ld_dst, ntap, shift0, dshift, Ti, ones_row):
    """Pure data movement: M and C no multiples of 64, ld_dst > M (zero padding), three taps with clip edges (one case with
    |shift| > Ti: all zero), the row of ones on and off; the row behind the last one stays untouched."""
    lib = _lib.load()
    rng = np.random.default_rng(M + C_)
    src = np.full((M, ld_src), to_bf16(np.float32(BIG)), np.float32)
    src[:, :C_] = to_bf16(rng.standard_normal((M, C_)))
    rows = ntap * C_ + ones_row
    want = np.zeros((rows, ld_dst), np.float32)
    for z in range(ntap):
        ok, s = tap_rows(M, shift0 + z * dshift, Ti, M)
        want[z * C_:(z + 1) * C_, :M] = np.where(ok[:, None], src[s, :C_], 0.0).T
    if ones_row:
        want[ntap * C_, :M] = 1.0
    d_src = bdev(src)
    dst = torch.full((rows * ld_dst + GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
    dst[:rows * ld_dst] = float("nan")
    _lib.check(lib.fwn_transpose_shift(d_src.data_ptr(), M, C_, ld_src, shift0, dshift, ntap, Ti, dst.data_ptr(), ld_dst, ones_row, stream()),
               "fwn_transpose_shift")
    torch.cuda.synchronize()
    assert bool((dst[rows * ld_dst:] == SENT).all())
    assert same_bits(dst[:rows * ld_dst].float().cpu().numpy().reshape(rows, ld_dst), want)
    assert np.array_equal(d_src[:src.size].float().cpu().numpy().reshape(src.shape), src)


# =================================================================== fwn_wn_backward_group
# (K, N, nsplit, row_src, col_src, col0, bias row, weight norm, scale): K = 1056 and 2080 make the middle pass loop twice
# and three times (33 and 65 row chunks); nsplit 1, 3, 4, 7: the 4-at-a-time loop and its 1 - 3 tail
WN_SPECS = [
    (1, 8, 1, False, False, 0, True, True, 1.0),
    (33, 72, 3, True, False, 0, True, True, 0.5),
    (768, 256, 4, False, False, 256, True, True, 0.7),
    (1056, 72, 7, False, True, 0, True, True, 1.0),
    (2080, 256, 3, True, True, 8, True, True, -1.3),
    (2080, 8, 4, False, False, 0, False, True, 1.0),
    (1056, 256, 1, True, False, 0, False, True, 2.0),
    (768, 72, 7, False, True, 16, True, False, 0.7),
    (33, 256, 4, True, True, 0, True, False, 1.0),
    (1, 72, 3, False, False, 0, False, False, 1.0),
    (1025, 8, 5, False, False, 0, True, True, 1.0),
    (1024, 8, 2, False, False, 0, True, True, 1.0),
    (33, 8, 6, True, False, 24, True, True, 1.0),
    (768, 8, 1, False, True, 0, True, True, 1.0),
    (100, 200, 3, False, False, 0, True, True, 1.0),
    (2080, 72, 7, True, True, 8, True, False, 0.25),
]


@pytest.mark.parametrize("njobs", [1, 5, 16])
def test_wn_backward_group_matches_fp64_reference(njobs):
    """The first njobs of WN_SPECS in one call (16 = FWN_MAX_GROUP; weight-normed and g = NULL jobs mixed): db, dV, dg within
    the bounds of the module docstring, db untouched where bias_row = -1, identical bits on a repeat; the partial matrices
    are taller and wider than what is read and hold 1e30 everywhere else."""
    lib = _lib.load()
    assert njobs <= _lib.FWN_MAX_GROUP == 16 == len(WN_SPECS)
    specs = WN_SPECS[-njobs:] if njobs == 5 else WN_SPECS[:njobs]
    rng = np.random.default_rng(njobs)
    arr = (_lib.WnJob * njobs)()
    refs, keep = [], []
    for q, (K, N, nsplit, rs, cs, col0, has_b, normed, scale) in zip(arr, specs):
        scale = float(np.float32(scale))
        rows, ldp = K + 6, col0 + N + 3
        row_src = rng.permutation(K + 5)[:K].astype(np.int32) if rs else None
        col_src = rng.permutation(N).astype(np.int32) if cs else None
        bias_row = K + 5 if has_b else -1
        part = np.full((nsplit, rows, ldp), BIG, np.float32)
        rr = np.arange(K) if row_src is None else row_src
        cc = col0 + (np.arange(N) if col_src is None else col_src)
        part[:, rr[:, None], cc[None, :]] = rng.standard_normal((nsplit, K, N)).astype(np.float32)
        if has_b:
            part[:, bias_row, cc] = rng.standard_normal((nsplit, N)).astype(np.float32)
        V = rng.standard_normal((K, N)).astype(np.float32)
        g = (rng.random(N) + 0.5).astype(np.float32)
        refs.append(ref_wn_backward(part, K, N, scale, row_src, col_src, col0, bias_row, V if normed else None, g if normed else None))
        d = dict(part=dev(part), V=dev(V), g=dev(g), rs=dev(row_src, 0) if rs else None, cs=dev(col_src, 0) if cs else None, host=(part, V, g))
        keep.append(d)
        q.part, q.split_stride, q.nsplit, q.ldp, q.col0, q.bias_row, q.K, q.N, q.scale = d["part"].data_ptr(), rows * ldp, nsplit, ldp, col0, bias_row, K, N, scale
        q.row_src, q.col_src = d["rs"].data_ptr() if rs else None, d["cs"].data_ptr() if cs else None
        q.V, q.g = (d["V"].data_ptr(), d["g"].data_ptr()) if normed else (None, None)
    nscr = int(lib.fwn_wn_group_scratch(arr, njobs))

    def run():
        outs = []
        for q, (K, N, *_rest) in zip(arr, specs):
            o = dict(dV=scratch(K * N), dg=scratch(N), db=scratch(N))
            q.dV, q.dg, q.db = o["dV"].data_ptr(), o["dg"].data_ptr(), o["db"].data_ptr()
            outs.append(o)
        scr = scratch(nscr, torch.float64)
        _lib.check(lib.fwn_wn_backward_group(arr, njobs, scr.data_ptr(), stream()), "fwn_wn_backward_group")
        torch.cuda.synchronize()
        assert guard_intact(scr, nscr)
        res = []
        for o, (K, N, *_rest) in zip(outs, specs):
            assert guard_intact(o["dV"], K * N) and guard_intact(o["dg"], N) and guard_intact(o["db"], N)
            res.append(dict(dV=host(o["dV"], (K, N)).copy(), dg=host(o["dg"], (N,)).copy(), db=host(o["db"], (N,)).copy()))
        return res

    res = run()
    for r, ref, d, (K, N, nsplit, rs, cs, col0, has_b, normed, scale) in zip(res, refs, keep, specs):
        delta = 2.0 * (nsplit + 2) * U * ref["dW_abs"]
        if has_b:
            note_ratio("wn db", r["db"], ref["db"], 2.0 * (nsplit + 2) * U * ref["db_abs"])
        else:
            assert np.isnan(r["db"]).all()                 # bias_row = -1: db untouched
        if not normed:
            note_ratio("wn dV (no norm)", r["dV"], ref["dV"], delta)
            assert np.isnan(r["dg"]).all()
            continue
        V64, g64, nrm = d["host"][1].astype(np.float64), d["host"][2].astype(np.float64), ref["nrm"]
        e_g = (delta * np.abs(V64)).sum(0) / nrm
        note_ratio("wn dg", r["dg"], ref["dg"], e_g + 2.0 * U * np.abs(ref["dg"]))
        note_ratio("wn dV", r["dV"], ref["dV"], np.abs(g64) / nrm * (delta + np.abs(V64) * e_g / nrm) + 2.0 * U * np.abs(ref["dV"]))
    res2 = run()
    assert all(same_bits(a[k], b[k]) for a, b in zip(res, res2) for k in ("dV", "dg", "db"))
    for d in keep:
        part, V, g = d["host"]
        assert guard_intact(d["part"], part.size) and same_bits(host(d["part"], part.shape), part) and same_bits(host(d["V"], V.shape), V)


# =================================================================== fwn_colsum_bf16
@pytest.mark.parametrize("M,C_,ld,blocks", [(1, 8, 8, 1), (511, 72, 80, 1), (512, 72, 80, 2), (1300, 200, 208, 5), (2600, 1100, 1104, 10)])
def test_colsum_bf16_matches_fp64_reference(M, C_, ld, blocks):
    """ld > C, C no multiple of 64, M on both sides of the step from one row block to two (511 | 512); scale != 1.  Bound: the
    module docstring."""
    lib = _lib.load()
    rng = np.random.default_rng(M + C_)
    dy = np.full((M, ld), to_bf16(np.float32(BIG)), np.float32)
    dy[:, :C_] = to_bf16(rng.standard_normal((M, C_)))
    scale = float(np.float32(-0.6))
    npart = int(lib.fwn_colsum_partials(M, C_))
    assert npart == blocks * C_
    per = (M + blocks - 1) // blocks
    d64 = dy[:, :C_].astype(np.float64)
    d_dy = bdev(dy)
    res = []
    for rep in range(2):
        part, out = scratch(npart), scratch(C_)
        _lib.check(lib.fwn_colsum_bf16(d_dy.data_ptr(), M, C_, ld, scale, part.data_ptr(), out.data_ptr(), stream()), "fwn_colsum_bf16")
        torch.cuda.synchronize()
        assert guard_intact(part, npart) and guard_intact(out, C_) and not bool(torch.isnan(part[:npart]).any())
        res.append(host(out, (C_,)).copy())
    note_ratio("colsum_bf16", res[0], scale * d64.sum(0), 2.0 * ((per + 3) // 4 + 2) * U * abs(scale) * np.abs(d64).sum(0))
    assert same_bits(res[0], res[1]) and guard_intact(d_dy, dy.size)


def test_zz_report_worst_ratios():
    """Not a check of its own: prints the worst err / bound of the bounded cases that ran in this session, per kernel and form."""
    for k in sorted(RATIOS):
        print("worst err / bound  %-36s %.3f" % (k, RATIOS[k]))
    assert all(v <= 1.0 for v in RATIOS.values())
