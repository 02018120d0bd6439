"""Ragged training step (-m gpu): ``GradEngine.loss_and_grads(..., lengths=)`` / ``Trainer.step(x, c, lengths=)`` give
loss = -(1/B) sum_b (log_p[b] + logdet[b]) over every clip's own samples and, for every trainable tensor, the mean over the
clips of that clip's own gradient - whatever the batch holds past a clip's end.

Cases A - D: each holds T itself and the shortest legal clip; C has two weight-gradient job groups per flow and a dilation of 27
that reaches past the short clips, D the ring front conv (Ch = 32) and the hoisted conditioning backward.  Bounds: the gradient
bounds are tests/test_train.py's (``grad_rel_allowed``, ``GRAD_*``, median 3e-2 / 4e-2 at full width, cosine > 0.999, dead
res conv exactly 0), copied by import; the scalar bounds are tests/test_ragged_forward.py's ``REL_LOGP`` / ``ABS_LOGDET``.
Statements about padding, repeated calls, full lengths and the recorded step are exact."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import small_hparams
from test_ragged_forward import ABS_LOGDET, BAD_LENGTHS, REL_LOGP, _ragged_inputs
from test_train import grad_rel_allowed                      # GRAD_REL / GRAD_FLOOR / GRAD_REL_MAX / GRAD_BIG live behind it
from test_train_stage_refs import ref_small_grads
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import training as TR
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd.training import GradEngine, Trainer

pytestmark = pytest.mark.gpu

CFG_B = dict(n_block=4, n_flow=2, n_layer=3, hop_size=32, upsample_scales=[4, 8], num_mels=16)
CASES = {
    "A": (dict(), 128, [128, 16, 64, 96]),
    "B": (CFG_B, 512, [512, 32, 288]),
    "C": (dict(n_block=4, n_flow=2, n_layer=4, hop_size=16, upsample_scales=[4, 4], num_mels=16), 512, [160, 512, 16]),
    "D": ("full6", 1024, [1024, 256]),
}
MEDIAN = {"A": 3e-2, "B": 3e-2, "C": 3e-2, "D": 4e-2}


def _hp(cfg):
    return default_hparams().replace(n_block=6) if cfg == "full6" else small_hparams(**cfg)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(name, junk=True):
    cfg, t, lengths = CASES[name]
    hp = _hp(cfg)
    unit = int(np.lcm(hp.hop_size, 1 << hp.n_block))
    assert t in lengths and unit in lengths                                   # T itself and the shortest legal clip
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk)
    return hp, t, lengths, x, c


def _params(hp, seed=None):
    """Random ActNorm tables (the -shift fill and the per-clip ActNorm terms must matter).  Default seeds: those of
    tests/test_train.py's oracle tests at the same widths - 5 for the small models, 1234 for the full-width one (case D)."""
    if seed is None:
        seed = 1234 if hp.num_mels == default_hparams().num_mels and hp.n_block >= 6 else 5
    return W.synthetic_params(hp, seed, actnorm="random")


def _run(eng, p, x, c, lengths, **kw):
    """One ragged call -> (loss, log_p, logdet, per-clip log_p, per-clip logdet, gradients), all copied out."""
    b, t = x.shape[0], x.shape[1]
    loss, lp, ld, g = eng.loss_and_grads(p, dev(x).reshape(b, t), dev(c), lengths=lengths, **kw)
    torch.cuda.synchronize()
    return (loss.clone(), lp.clone(), ld.clone(), eng.per_clip[0].clone(), eng.per_clip[1].clone(), {k: v.clone() for k, v in g.items()})


_ORACLE = {}


def _oracle(name):
    """fp64 autograd of every clip on its own (oracle/grad_torch.py), computed once per case: per-clip (loss, log_p, logdet)
    and the mean over the clips of the per-clip gradients."""
    if name not in _ORACLE:
        from oracle import grad_torch as G
        hp, t, lengths, x, c = _case(name)
        p = _params(hp)
        per, mean = [], None
        for k, n in enumerate(lengths):
            loss, lp, ld, g = G.loss_and_grads(p, x[k:k + 1, :n], c[k:k + 1, :n // hp.hop_size], hp)
            per.append((loss, lp, ld))
            mean = {q: v / len(lengths) for q, v in g.items()} if mean is None else {q: mean[q] + g[q] / len(lengths) for q in mean}
        _ORACLE[name] = (per, mean)
    return _ORACLE[name]


def _check_scalars(got, per):
    """Per-clip log_p / logdet to tests/test_ragged_forward.py's bounds; the batch means and the loss to the same bounds at the
    means (the loss is minus the sum of the two, so its bound is the sum of theirs)."""
    loss, lp, ld, lpb, ldb = got[:5]
    for k, (loss0, lp0, ld0) in enumerate(per):
        print("clip %d: log_p %.6f (oracle %.6f)  logdet %.6f (oracle %.6f)" % (k, float(lpb[k]), lp0, float(ldb[k]), ld0))
        assert abs(float(lpb[k]) - lp0) <= REL_LOGP * abs(lp0), (k, float(lpb[k]), lp0)
        assert abs(float(ldb[k]) - ld0) <= ABS_LOGDET * max(1.0, abs(ld0)), (k, float(ldb[k]), ld0)
    loss0, lp0, ld0 = (float(np.mean([v[i] for v in per])) for i in range(3))
    b_lp, b_ld = REL_LOGP * abs(lp0), ABS_LOGDET * max(1.0, abs(ld0))
    print("loss %.6f (oracle %.6f)  mean log_p %.6f (%.6f)  mean logdet %.6f (%.6f)" % (float(loss), loss0, float(lp), lp0, float(ld), ld0))
    assert abs(float(lp) - lp0) <= b_lp and abs(float(ld) - ld0) <= b_ld
    assert abs(float(loss) - loss0) <= b_lp + b_ld, (float(loss), loss0)


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_are_the_mean_of_the_per_clip_oracle_gradients(name):
    hp, t, lengths, x, c = _case(name)
    per, g0 = _oracle(name)
    got = _run(GradEngine(hp), _params(hp), x, c, lengths)
    _check_scalars(got, per)
    g = got[5]
    assert sorted(g) == sorted(g0)
    total = float(np.sqrt(sum(float((v * v).sum()) for v in g0.values())))
    rels, dot, na, nb_ = [], 0.0, 0.0, 0.0
    for k in sorted(g0):
        a, r = g[k].cpu().numpy().astype(np.float64).reshape(-1), np.asarray(g0[k], dtype=np.float64).reshape(-1)
        assert np.isfinite(a).all(), k
        if "res_conv" in k and ("ResBlock_%d/" % (hp.n_layer - 1)) in k:
            assert not a.any() and not r.any(), k          # dead conv (modules.py:126-128): zero gradient
            continue
        nr = np.linalg.norm(r)
        rel = np.linalg.norm(a - r) / nr
        rels.append(rel)
        assert rel < grad_rel_allowed(nr, total, rel), (k, rel, nr, total)
        dot += float(a @ r); na += float(a @ a); nb_ += float(r @ r)
    print("case %s: median relative error %.4f, worst %.4f, cosine %.6f" % (name, np.median(rels), max(rels), dot / np.sqrt(na * nb_)))
    assert np.median(rels) < MEDIAN[name], np.median(rels)
    assert dot / np.sqrt(na * nb_) > 0.999


# ------------------------------------------------------------------ 2. padding is inert
@pytest.mark.parametrize("name", list(CASES))
def test_padding_is_inert_bit_for_bit(name):
    hp = _case(name)[0]
    p = _params(hp)
    eng = GradEngine(hp)
    outs = []
    for junk in (False, True, True):
        hp, t, lengths, x, c = _case(name, junk)
        b = len(lengths)
        xd, cd, ld_ = dev(x).reshape(b, t), dev(c), torch.tensor(lengths, dtype=torch.int32).cuda()
        keep = (xd.clone(), cd.clone(), ld_.clone())
        loss, lp, ld, g = eng.loss_and_grads(p, xd, cd, lengths=ld_)
        torch.cuda.synchronize()
        assert torch.equal(xd, keep[0]) and torch.equal(cd, keep[1]) and torch.equal(ld_, keep[2])     # the caller's tensors are never written
        outs.append((loss.clone(), lp.clone(), ld.clone(), eng.per_clip[0].clone(), eng.per_clip[1].clone(), {k: v.clone() for k, v in g.items()}))
    for o in outs:
        assert all(bool(torch.isfinite(v).all()) for v in o[:5]) and all(bool(torch.isfinite(v).all()) for v in o[5].values())
        assert o[3].shape == o[4].shape == (len(lengths),)
    for other in outs[1:]:          # zeros against junk, and the same call again
        for a, b_ in zip(outs[0][:5], other[:5]):
            assert torch.equal(a, b_)
        for k in outs[0][5]:
            assert torch.equal(outs[0][5][k], other[5][k]), k
    assert any(bool(v.any()) for v in outs[0][5].values())


# ------------------------------------------------------------------ 3. full lengths
@pytest.mark.parametrize("name", list(CASES))
def test_full_lengths_give_the_plain_step_bit_for_bit(name):
    cfg, t, lengths = CASES[name]
    hp, b = _hp(cfg), len(lengths)
    p = _params(hp, 21)
    inp = W.synthetic_inputs(hp, b, t, want=("x", "c"))
    x, c = dev(inp["x"]).reshape(b, t), dev(inp["c"])
    eng = GradEngine(hp)
    loss0, lp0, ld0, g0 = eng.loss_and_grads(p, x, c)
    torch.cuda.synchronize()
    assert eng.per_clip is None
    loss0, lp0, ld0, g0 = float(loss0), float(lp0), float(ld0), {k: v.clone() for k, v in g0.items()}
    loss, lp, ld, g = eng.loss_and_grads(p, x, c, lengths=[t] * b)
    torch.cuda.synchronize()
    for k in g0:
        assert torch.equal(g[k], g0[k]), k
    # the scalars' reduction order differs (per clip, fp64): within the bounds of the oracle test
    b_lp, b_ld = REL_LOGP * abs(lp0), ABS_LOGDET * max(1.0, abs(ld0))
    assert abs(float(lp) - lp0) <= b_lp and abs(float(ld) - ld0) <= b_ld and abs(float(loss) - loss0) <= b_lp + b_ld
    assert abs(float(eng.per_clip[0].double().mean()) - lp0) <= b_lp and abs(float(eng.per_clip[1].double().mean()) - ld0) <= b_ld
    again = eng.loss_and_grads(p, x, c)                      # the plain step is untouched by the ragged one before it
    torch.cuda.synchronize()
    assert (float(again[0]), float(again[1]), float(again[2])) == (loss0, lp0, ld0)
    assert all(torch.equal(again[3][k], g0[k]) for k in g0)


# ------------------------------------------------------------------ 4. recorded equals eager, side stream equals one stream
def test_recorded_step_equals_eager_step_and_reads_the_lengths_at_replay():
    hp = small_hparams(**CFG_B)
    t = 512
    la, lb = [512, 32, 288], [64, 512, 160]
    xa, ca = _ragged_inputs(hp, 3, t, la, True)
    xb, cb = _ragged_inputs(hp, 3, t, lb, True)
    steps = [(xa, ca, la)] * 3 + [(xb, cb, lb), (xa, ca, la)]
    runs = {}
    for graph in (False, True):
        tr = Trainer(hp, _params(hp, 11), graph=graph)
        outs, w3 = [], None
        for n, (x, c, lens) in enumerate(steps):
            out = tr.step(dev(x).reshape(3, t), dev(c), lengths=lens)
            outs.append(tuple(float(v) for v in out) + tuple(tr.per_clip[0].tolist()) + tuple(tr.per_clip[1].tolist()))
            if n == 2:
                w3 = tr.opt.w.clone()
        assert tr.graph is graph                             # the recording did not fall back to eager steps
        runs[graph] = (outs, w3, tr.opt.w.clone())
        if graph:
            assert len([k for k, v in tr._recorded.items() if isinstance(v, dict)]) == 1          # one recording serves every batch
    assert all(np.isfinite(v) for o in runs[True][0] for v in o)
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1])        # masters after 3 steps
    assert torch.equal(runs[True][2], runs[False][2])        # and after the replays with other lengths
    assert runs[True][0][3] != runs[True][0][2]


def test_side_stream_and_one_stream_engines_agree_bit_for_bit():
    hp, t, lengths, x, c = _case("B")
    p = _params(hp, 23)
    res = {}
    for side in (False, True):
        eng = GradEngine(hp, side_stream=side)
        order = []
        for rep in range(2):
            order.clear()
            out = _run(eng, p, x, c, lengths, on_block_done=order.append)
        assert order == list(range(hp.n_block - 1, -1, -1)) + [-1]
        res[side] = out
    for a, b in zip(res[False][:5], res[True][:5]):
        assert torch.equal(a, b)
    for k in res[False][5]:
        assert torch.equal(res[False][5][k], res[True][5][k]), k


# ------------------------------------------------------------------ 5. stage level
def bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.bfloat16)


# (clips, Ti, rows kept per clip): the issue's shape (32 x 64 tiles, direct epilogue) and one of 64 x 128 tiles (row epilogue)
@pytest.mark.parametrize("clips,ti,keep", [(3, 40, [40, 1, 17]), (3, 1000, [1000, 1, 417])])
def test_gemm_length_fields_zero_the_rows_past_each_clip(clips, ti, keep):
    rng = np.random.default_rng(ti)
    m, n, spr = clips * ti, 256, 4
    x = bf(rng.standard_normal((m, 256)) * 0.5)
    w = bf(rng.standard_normal((n, 768)) * 0.05)
    res, mask = bf(rng.standard_normal((m, n))), bf(rng.standard_normal((m, n)) + 1.0)
    segs = [(x, 256, -9, 0), (x, 256, 0, 256), (x, 256, 9, 512)]
    lens = torch.tensor([k * spr for k in keep], dtype=torch.int32).cuda()
    padded = np.concatenate([np.arange(ti) >= k for k in keep])
    assert padded.any() and not padded.all()
    for kw in (dict(), dict(res=res, rscale=0.7, mask=mask), dict(out_f32=True)):
        plain = TR.gemm(segs, w, n, m, ti=ti, **kw)
        got = TR.gemm(segs, w, n, m, ti=ti, row_len=(lens, spr), **kw)
        again = TR.gemm(segs, w, n, m, ti=ti, **kw)          # a NULL pointer: today's bits
        torch.cuda.synchronize()
        assert torch.equal(again, plain)
        pd = torch.from_numpy(padded).cuda()
        assert bool(plain[pd].any())                         # the product itself is not 0 there
        assert not bool(got[pd].any())                       # exactly 0 past each end
        assert torch.equal(got[~pd], plain[~pd])             # every other row: the call without lengths
    with pytest.raises(RuntimeError, match="accumulate"):
        TR.gemm(segs, w, n, m, ti=ti, row_len=(lens, spr), out=torch.zeros(m, n, device="cuda"), accumulate=True)


def _stage_case(clips, rows, ch, keep):
    rng = np.random.default_rng(clips * rows + ch)
    m = clips * rows
    valid = np.concatenate([np.arange(rows) < k for k in keep])
    lens = torch.tensor([k * 2 * ch for k in keep], dtype=torch.int32).cuda()
    return rng, m, valid, lens


STAGE = [(3, 11, 8, [11, 1, 6]), (2, 5, 128, [5, 2])]


@pytest.mark.parametrize("clips,rows,ch,keep", STAGE)
def test_coupling_bwd_ragged_matches_numpy(clips, rows, ch, keep):
    """fwn_coupling_bwd_ragged against fp64 NumPy, tolerances of tests/test_train.py::test_elementwise_stage_entry_points_match_numpy;
    the rows past a clip's end hold NaN on the way in (a read of them would show) and exact zeros on the way out."""
    lib = _lib.load()
    rng, m, valid, lens = _stage_case(clips, rows, ch, keep)
    st = torch.cuda.current_stream().cuda_stream
    Z = (rng.standard_normal((m, 2 * ch)) * 0.3).astype(np.float32)
    ez = np.exp(rng.standard_normal(2 * ch) * 0.1).astype(np.float32)
    g, ob, ya = (rng.standard_normal((m, ch)).astype(np.float32) for _ in range(3))
    for a in (Z, g, ob, ya):
        a[~valid] = np.nan
    ldz, ldya = max(8, 2 * ch), max(8, ch)
    dg, dob, dZ_, dez, dya = dev(g), dev(ob), dev(Z), dev(ez), dev(ya)
    dz = torch.full((m, ldz), 7.0, device="cuda", dtype=torch.bfloat16)
    dzz = torch.full((m, 2 * ch), 7.0, device="cuda")
    yabf = torch.full((m, ldya), 7.0, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.fwn_coupling_bwd_ragged(dg.data_ptr(), dob.data_ptr(), dZ_.data_ptr(), dez.data_ptr(), clips, rows, ch, lens.data_ptr(), 2 * ch,
                                           dz.data_ptr(), ldz, dzz.data_ptr(), dya.data_ptr(), yabf.data_ptr(), ldya, st), "fwn_coupling_bwd_ragged")
    torch.cuda.synchronize()
    cls = np.repeat([1.0 / (clips * k * 2 * ch) for k in keep], rows)[:, None]           # 1 / (B len[b]) per row
    ls, t = Z[:, :ch].astype(np.float64) * ez[:ch], Z[:, ch:].astype(np.float64) * ez[ch:]
    e = np.exp(-ls)
    dls, dt = -g * ob + cls, -g * e
    want = dict(g=g * e, ob=ob / e + t, dz=np.concatenate([dls * ez[:ch], dt * ez[ch:]], 1), dzz=np.concatenate([dls * ls, dt * t], 1), ya=ya.astype(np.float64))
    got = dict(g=dg, ob=dob, dz=dz[:, :2 * ch].float(), dzz=dzz, ya=yabf[:, :ch].float())
    tol = dict(g=1e-5, ob=2e-5, dz=1e-2, dzz=1e-4, ya=1e-2)                               # dz and ya are bf16
    for k in want:
        a, r = got[k].cpu().numpy().astype(np.float64), want[k]
        assert not a[~valid].any(), k                                                     # exactly 0 past each clip's end
        assert np.abs(a[valid] - r[valid]).max() <= tol[k] * max(1.0, np.abs(r[valid]).max()), k
    assert not dz[:, 2 * ch:].float().cpu().numpy().any() and not yabf[:, ch:].float().cpu().numpy().any()      # zero padding of the rows
    # full lengths: the bits of the plain kernel
    Zf, gf, obf = np.nan_to_num(Z, nan=0.25), np.nan_to_num(g, nan=0.5), np.nan_to_num(ob, nan=-0.5)
    outs = []
    for ragged in (False, True):
        a, b_, zf = dev(gf), dev(obf), dev(Zf)
        dz2, dzz2 = torch.zeros(m, ldz, device="cuda", dtype=torch.bfloat16), torch.zeros(m, 2 * ch, device="cuda")
        if ragged:
            full = torch.tensor([rows * 2 * ch] * clips, dtype=torch.int32).cuda()
            _lib.check(lib.fwn_coupling_bwd_ragged(a.data_ptr(), b_.data_ptr(), zf.data_ptr(), dez.data_ptr(), clips, rows, ch, full.data_ptr(),
                                                   2 * ch, dz2.data_ptr(), ldz, dzz2.data_ptr(), None, None, 0, st), "fwn_coupling_bwd_ragged")
        else:
            _lib.check(lib.fwn_coupling_bwd(a.data_ptr(), b_.data_ptr(), zf.data_ptr(), dez.data_ptr(), m, ch,
                                            float(np.float32(1.0 / (2.0 * m * ch))), dz2.data_ptr(), ldz, dzz2.data_ptr(), st), "fwn_coupling_bwd")
        torch.cuda.synchronize()
        outs.append((a, b_, dz2, dzz2))
    assert all(torch.equal(p_, q) for p_, q in zip(*outs))


@pytest.mark.parametrize("clips,rows,ch,keep", STAGE)
def test_small_grads_ragged_match_numpy(clips, rows, ch, keep):
    """fwn_flow_small_grads_ragged: the five sums over the clips' own rows only (NaN in every other row on the way in), the four
    planes exactly 0 past each clip's end and fwn_flow_small_grads' values inside."""
    lib = _lib.load()
    rng, m, valid, lens = _stage_case(clips, rows, ch, keep)
    st = torch.cuda.current_stream().cuda_stream
    an = rng.standard_normal((2, 4, ch)).astype(np.float32) * 0.3
    an[:, 1] = np.exp(an[:, 1]); an[:, 2] = 1.0 / an[:, 1]
    ga, ya, gb, yb = (rng.standard_normal((m, ch)).astype(np.float32) for _ in range(4))
    dzz = rng.standard_normal((m, 2 * ch)).astype(np.float32)
    for a in (ga, ya, gb, yb, dzz):
        a[~valid] = np.nan
    br, zc = rng.permutation(ch).astype(np.int64), rng.permutation(2 * ch).astype(np.int64)
    ref = ref_small_grads(ga[valid], ya[valid], gb[valid], yb[valid], dzz[valid], an, br, zc)
    planes = [dev(a) for a in (ga, ya, gb, yb)]
    outs = [torch.full((2 * ch,), float("nan"), device="cuda") for _ in range(3)]
    part = torch.empty(int(lib.fwn_flow_small_grads_partials(m, ch)), dtype=torch.float64, device="cuda")
    d_dzz, d_an, d_br, d_zc = dev(dzz), dev(an), dev(br), dev(zc)
    _lib.check(lib.fwn_flow_small_grads_ragged(*[p_.data_ptr() for p_ in planes], d_dzz.data_ptr(), d_an.data_ptr(), clips, rows, ch, lens.data_ptr(),
                                               2 * ch, d_br.data_ptr(), d_zc.data_ptr(), part.data_ptr(), *[o.data_ptr() for o in outs], st),
               "fwn_flow_small_grads_ragged")
    torch.cuda.synchronize()
    for name, o in zip(("db", "dlogs", "dzscale"), outs):
        a = o.cpu().numpy().astype(np.float64)
        assert np.isfinite(a).all(), name                                                 # no padded row was summed
        assert np.abs(a - ref[name]).max() <= 1e-4 * max(1.0, ref[name + "_abs"].max()), name
    for a, key in zip(planes, ("g0", "x0", "g1", "x1")):
        a = a.cpu().numpy().astype(np.float64)
        assert not a[~valid].any(), key                                                   # exactly 0 in all four planes
        assert np.abs(a[valid] - ref[key]).max() <= 1e-5 * max(1.0, np.abs(ref[key]).max()), key


# ------------------------------------------------------------------ 6. errors
def test_refusals():
    hp = small_hparams()
    p = _params(hp)
    inp = W.synthetic_inputs(hp, 3, 64, want=("x", "c"))
    x, c = dev(inp["x"]).reshape(3, 64), dev(inp["c"])
    eng = GradEngine(hp)
    first = eng.loss_and_grads(p, x, c, lengths=[64, 16, 48])          # kept: the descriptors point at these gradient tensors
    torch.cuda.synchronize()
    l0 = float(first[0])

    class NoLaunch:             # any call into the library (or a refresh of the packing) during a refused call would show
        def __getattr__(self, name):
            raise AssertionError("libfwn.%s reached with bad lengths" % name)

    def no_refresh():
        raise AssertionError("the packing was refreshed with bad lengths")

    real, refresh = eng.lib, eng._tp.refresh
    eng.lib, eng._tp.refresh = NoLaunch(), no_refresh
    try:
        for bad in BAD_LENGTHS:
            with pytest.raises(ValueError):
                eng.loss_and_grads(p, x, c, lengths=bad)
    finally:
        eng.lib, eng._tp.refresh = real, refresh
    tr = Trainer(hp, p, graph=False)
    w0 = tr.opt.w.clone()
    for bad in BAD_LENGTHS:
        with pytest.raises(ValueError):
            tr.step(x, c, lengths=bad)
    assert torch.equal(tr.opt.w, w0) and tr.opt.global_step == 0
    with pytest.raises(ValueError, match="gate_fp8"):
        GradEngine(hp.replace(gate_fp8=True)).loss_and_grads(p, x, c, lengths=[64, 16, 48])
    # the C entry point refuses null lengths and a short workspace by itself, with a message and without a launch
    lib, td = eng.lib, eng._desc
    need = int(lib.fwn_train_ragged_workspace_bytes(C.byref(td), 3, 64))
    assert need > int(lib.fwn_train_workspace_bytes(C.byref(td), 3, 64)) > 0
    assert int(lib.fwn_train_ragged_workspace_bytes(C.byref(td), 3, 60)) == 0 and int(lib.fwn_train_ragged_workspace_bytes(C.byref(td), 40000, 64)) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    out3 = torch.zeros(3, device="cuda")
    lens = torch.tensor([64, 16, 48], dtype=torch.int32).cuda()
    cb = _lib.BLOCK_DONE_FN(lambda user, blk: 0)
    call = lambda lp_, wsn: lib.fwn_train_loss_and_grads_ragged(C.byref(td), 3, 64, x.data_ptr(), c.data_ptr(), lp_, base, wsn, out3.data_ptr(), None, cb,
                                                              None, None)
    assert call(None, need) == -1 and b"null lengths" in lib.fwn_last_error()
    assert call(lens.data_ptr(), need - 1) == -3 and b"workspace" in lib.fwn_last_error()
    torch.cuda.synchronize()
    assert float(out3.abs().sum()) == 0.0                       # nothing ran
    assert call(lens.data_ptr(), need) == 0                     # out2B may be NULL
    torch.cuda.synchronize()
    assert float(out3[0]) == l0
    # fwn_gemm: the length fields together with accumulate
    g = _lib.GemmDesc()
    buf = torch.zeros(64, 64, device="cuda")
    xb = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    g.W, g.Y, g.nseg, g.M, g.N, g.Ti, g.ldw, g.ldy, g.nsplit, g.out_f32 = xb.data_ptr(), buf.data_ptr(), 1, 64, 64, 32, 64, 64, 1, 1
    g.seg[0].x, g.seg[0].rows, g.seg[0].ld, g.seg[0].k = xb.data_ptr(), 64, 64, 64
    g.row_len, g.len_spr, g.accumulate = lens.data_ptr(), 2, 1
    assert lib.fwn_gemm(C.byref(g), None) == -1 and b"accumulate" in lib.fwn_last_error()
    g.accumulate, g.Ti = 0, 0
    assert lib.fwn_gemm(C.byref(g), None) == -1 and b"row_len" in lib.fwn_last_error()
    assert lib.fwn_coupling_bwd_ragged(None, None, None, None, 2, 4, 1, None, 2, None, 8, None, None, None, 0, None) == -1
    assert lib.fwn_flow_small_grads_ragged(*([None] * 6), 2, 4, 1, None, 2, *([None] * 7)) == -1


# ------------------------------------------------------------------ 7. two ranks
DP_LENGTHS = [512, 32, 288, 160]


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)             # gloo moves CUDA tensors through the host; both ranks share cuda:0
    torch.cuda.set_device(0)
    hp = small_hparams(**CFG_B)
    x, c = _ragged_inputs(hp, 4, 512, DP_LENGTHS, True)
    lo = 2 * rank
    tr = Trainer(hp, _params(hp, 11), graph=False)
    tr.step(dev(x[lo:lo + 2]).reshape(2, 512), dev(c[lo:lo + 2]), lengths=DP_LENGTHS[lo:lo + 2])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), g=tr.opt.g.cpu().numpy(), w=tr.opt.w.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ragged_step_matches_one_process_on_the_whole_batch(tmp_path):
    """Two gloo ranks, two clips each: the all-reduced gradient is world x the gradient of the four-clip ragged batch in one
    process (the average of per-rank means over equally many clips is the mean over all clips) - to the bound of
    tests/test_train.py::test_two_rank_data_parallel_step_matches_one_process_on_the_whole_batch - and both ranks end the step
    with identical weights."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path)), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=150)
        codes = [p.exitcode for p in procs]
    finally:
        for p in procs:             # a rank that died leaves its peer waiting in a collective: never leave it behind
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert codes == [0, 0], codes
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2))
    assert np.array_equal(r0["g"], r1["g"]) and np.array_equal(r0["w"], r1["w"])
    hp = small_hparams(**CFG_B)
    x, c = _ragged_inputs(hp, 4, 512, DP_LENGTHS, True)
    tr = Trainer(hp, _params(hp, 11), graph=False)
    _, _, _, grads = tr.engine.loss_and_grads(tr.opt.master_views(), dev(x).reshape(4, 512), dev(c), lengths=DP_LENGTHS)
    gv = tr.opt.grad_views()
    for k, g in grads.items():
        gv[k].copy_(g.reshape(gv[k].shape))
    want, got = 2.0 * tr.opt.g.cpu().numpy().astype(np.float64), r0["g"].astype(np.float64)
    cos = float((want * got).sum() / np.sqrt((want * want).sum() * (got * got).sum()))
    print("cosine %.6f, norm ratio %.5f" % (cos, np.linalg.norm(got) / np.linalg.norm(want)))
    assert cos > 0.999 and abs(np.linalg.norm(got) / np.linalg.norm(want) - 1.0) < 2e-2, (cos, np.linalg.norm(got), np.linalg.norm(want))
