"""Ragged ActNorm data-dependent init (-m gpu): ``FloWaveNet.forward_init(x, c, lengths)`` derives every flow's ``b`` / ``logs``
from the union of the clips' own rows - nothing past a clip's end is read or counted - and then runs the flow as the ragged
forward runs it.

Reference: the fp64 composition of oracle/flowavenet_np.py in ``oracle_ragged_init`` below - one state per clip, each alone at
its own length; per flow ``actnorm_ddi`` on the clips' rows concatenated, then ``flow_forward(init=False)`` per clip.  Cases:
``SMALL`` of tests/test_ragged_forward.py.  Bounds: that file's ``REL_LOGP`` / ``ABS_LOGDET`` / ``ABS_Z`` (copied by import) for
the per-clip outputs; for the tables 2e-2 (``b``) and 5e-3 (``logs``), what tests/test_gpu_parity.py holds the last flow of a DDI
golden to - here for every flow; ``Block_0/Flow_0``, which depends on x alone, rtol 1e-5 / atol 1e-6
(``test_actnorm_ddi_kernel``'s).  Statements about the padding, repeated calls and the row count are exact."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import small_hparams
from oracle import flowavenet_np as onp
from test_ragged_forward import ABS_LOGDET, ABS_Z, BAD_LENGTHS, REL_LOGP, SMALL, _hp, _planes_past_the_end, _ragged_inputs, check_scalars
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.model import FloWaveNet, z_planes_to_squeezed
from tf_flowavenet_amd.training import Trainer

pytestmark = pytest.mark.gpu
ABS_B, ABS_LOGS = 2e-2, 5e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def flow_names(hp):
    return ["Block_%d/Flow_%d" % (i, j) for i in range(hp.n_block) for j in range(hp.n_flow)]


def oracle_ragged_init(params, x, c, lengths, hp, count_all_rows_of=None, first_flow_only=False):
    """-> (p64 with every ActNorm initialised, per-clip log_p, per-clip logdet, per-clip z).  count_all_rows_of = T: the means
    divide by all B x rows rows of a batch padded to T (zeros appended: the sums are the valid rows') - the wrong count.
    first_flow_only: stop behind the init of Block_0/Flow_0 and return p64 alone."""
    p = onp.to_f64(params)
    outs = [x[k:k + 1, :n].astype(np.float64) for k, n in enumerate(lengths)]
    cs = [onp.upsample(p, c[k:k + 1, :n // hp.hop_size].astype(np.float64), hp) for k, n in enumerate(lengths)]
    logdet = [0.0] * len(lengths)
    for i in range(hp.n_block):
        outs, cs = [onp.squeeze(o) for o in outs], [onp.squeeze(v) for v in cs]
        for j in range(hp.n_flow):
            prefix = "Block_%d/Flow_%d" % (i, j)
            cat = np.concatenate(outs, axis=1)
            if count_all_rows_of is not None:
                rows = len(lengths) * (count_all_rows_of >> (i + 1))
                cat = np.concatenate([cat, np.zeros((1, rows - cat.shape[1], cat.shape[2]))], axis=1)
            onp.actnorm_ddi(p, prefix + "/ActNorm", cat)
            if first_flow_only:
                return p
            for k in range(len(lengths)):
                outs[k], cs[k], det = onp.flow_forward(p, prefix, outs[k], cs[k], hp, init=False)
                logdet[k] += det
    log_p = [float(np.mean(0.5 * (-math.log(2.0 * math.pi) - np.square(o)))) for o in outs]
    return p, log_p, [float(v) for v in logdet], outs


_ORACLE = {}


def _case(k, junk=True):
    cfg, t, lengths = SMALL[k]
    hp = _hp(cfg)
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk)
    return hp, t, lengths, x, c


def _oracle(k):
    """The reference of case k, computed once (0.7 - 1.7 s in fp64) and left unchanged."""
    if k not in _ORACLE:
        hp, t, lengths, x, c = _case(k)
        _ORACLE[k] = oracle_ragged_init(W.synthetic_params(hp, 99, actnorm="zeros"), x, c, lengths, hp)
    return _ORACLE[k]


def _fresh(hp, **kw):
    return FloWaveNet(hp, **kw).load_params(W.synthetic_params(hp, 99, actnorm="zeros"))


def check_tables(an, p64, hp, what=""):
    worst_b = worst_l = 0.0
    for name in flow_names(hp):
        eb = float(np.abs(np.ravel(an[name + "/ActNorm/b"]) - np.ravel(p64[name + "/ActNorm/b"])).max())
        el = float(np.abs(np.ravel(an[name + "/ActNorm/logs"]) - np.ravel(p64[name + "/ActNorm/logs"])).max())
        worst_b, worst_l = max(worst_b, eb), max(worst_l, el)
        assert eb <= ABS_B and el <= ABS_LOGS, (what, name, eb, el)
    print("%s tables: worst b err %.3e (bound %.0e), worst logs err %.3e (bound %.0e)" % (what, worst_b, ABS_B, worst_l, ABS_LOGS))


# ------------------------------------------------------------------ 1. the moments kernel alone
def _moments(lib, xa, xb, clips, rows, ch, lens_dev, spr, offset=0, fill=float("nan")):
    """One call -> mom [4 ch + 1] fp64 (NumPy).  xa, xb: device buffers whose planes start `offset` floats in."""
    need = lib.fwn_actnorm_moments_ragged_scratch_bytes(clips, rows, ch)
    assert need > 0 and need % 8 == 0
    scratch = torch.full((need // 8,), fill, dtype=torch.float64, device="cuda")
    mom = torch.full((4 * ch + 1,), fill, dtype=torch.float64, device="cuda")
    rc = lib.fwn_actnorm_moments_ragged(xa.data_ptr() + 4 * offset, xb.data_ptr() + 4 * offset, clips, rows, ch, lens_dev.data_ptr(), spr,
                                        mom.data_ptr(), scratch.data_ptr(), need, None)
    assert rc == 0, lib.fwn_last_error()
    return mom.cpu().numpy()


def _moments_case(lib, clips, rows, ch, lens, offset=0):
    spr = 2 * ch
    rng = np.random.default_rng(rows * 29 + ch)
    planes = [(3.0 * rng.standard_normal((clips, rows, ch)) + 1.0).astype(np.float32),        # test_actnorm_ddi_kernel's scales
              (0.2 * rng.standard_normal((clips, rows, ch)) - 4.0).astype(np.float32)]
    keep = [min(max(v, 0) // spr, rows) for v in lens]
    for pl in planes:
        for k, r in enumerate(keep):
            pl[k, r:] = np.nan                                                  # a padded row read into a sum would show
    devs = [dev(np.concatenate([np.zeros(offset, dtype=np.float32), pl.reshape(-1)])) for pl in planes]
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    got = _moments(lib, devs[0], devs[1], clips, rows, ch, ld, spr, offset)
    again = _moments(lib, devs[0], devs[1], clips, rows, ch, ld, spr, offset, fill=0.0)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))           # fixed-order sums: the same bits again
    assert np.isfinite(got).all(), (rows, ch, lens)
    n = sum(keep)
    assert got[4 * ch] == float(n), (got[4 * ch], n)                            # the count is exact
    for role, pl in enumerate(planes):
        v = np.concatenate([pl[k, :r].astype(np.float64) for k, r in enumerate(keep)], axis=0)
        s, s2 = v.sum(0), (v * v).sum(0)
        es = np.abs(got[role * 2 * ch:role * 2 * ch + ch] - s) / np.maximum(np.abs(v).sum(0), 1e-300)
        es2 = np.abs(got[role * 2 * ch + ch:role * 2 * ch + 2 * ch] - s2) / np.maximum(s2, 1e-300)
        assert es.max() <= 1e-12 and es2.max() <= 1e-12, (rows, ch, role, es.max(), es2.max())
    # the tables fwn_actnorm_from_moments derives from them, against masked NumPy
    an = torch.empty(2, 4, ch, device="cuda")
    rc = lib.fwn_actnorm_from_moments(dev(got).data_ptr(), ch, an.data_ptr(), None)
    assert rc == 0, lib.fwn_last_error()
    for role, pl in enumerate(planes):
        v = np.concatenate([pl[k, :r].astype(np.float64) for k, r in enumerate(keep)], axis=0)
        mean = v.mean(0)
        den = np.sqrt(((v - mean) ** 2).mean(0)) + 1e-7
        t = an[role].cpu().numpy()
        np.testing.assert_allclose(t[0], -mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t[1], 1 / den, rtol=1e-5)
        np.testing.assert_allclose(t[2], den, rtol=1e-5)
        np.testing.assert_allclose(t[3], -np.log(den), rtol=1e-5, atol=1e-6)
    return got


def test_moments_kernel_alone():
    lib = _lib.load()
    for ch in (1, 2, 16, 128):
        rows, spr = 37, 2 * ch
        # len 0, the whole plane, past it (clamped), one row, all but one row, negative
        lens = [0, rows * spr, rows * spr + 1000, spr, (rows - 1) * spr, -5]
        _moments_case(lib, 6, rows, ch, lens)
        _moments_case(lib, 6, rows, ch, lens, offset=1)                         # a base that is not 16-byte aligned
    # more than one workgroup per channel
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(3, 70001, 1) > 4 * 8 and lib.fwn_actnorm_moments_ragged_scratch_bytes(2, 3000, 64) > 4 * 64 * 8
    _moments_case(lib, 3, 70001, 1, [2, 140002, 70000])
    _moments_case(lib, 3, 33333, 2, [4, 133332, 40004])
    _moments_case(lib, 2, 3000, 64, [128 * 2999, 128 * 1500])


def test_moments_of_full_lengths_are_the_plain_kernels():
    lib = _lib.load()
    for clips, rows, ch in ((4, 37, 1), (3, 1000, 8), (2, 3000, 64), (3, 33333, 2)):
        m = clips * rows
        g = torch.Generator().manual_seed(rows + ch)
        xa = (torch.randn(m, ch, generator=g) * 3 + 1).cuda()
        xb = (torch.randn(m, ch, generator=g) * 0.2 - 4).cuda()
        plain = torch.empty(4 * ch + 1, dtype=torch.float64, device="cuda")
        assert lib.fwn_actnorm_moments(xa.data_ptr(), xb.data_ptr(), m, ch, plain.data_ptr(), None) == 0
        ld = torch.full((clips,), rows * 2 * ch, dtype=torch.int32).cuda()
        got, want = _moments(lib, xa, xb, clips, rows, ch, ld, 2 * ch), plain.cpu().numpy()
        assert got[4 * ch] == want[4 * ch] == float(m)
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print("clips %d rows %d Ch %d: worst relative difference %.3e" % (clips, rows, ch, rel.max()))
        assert rel.max() <= 1e-12


def test_moments_entry_refuses_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(64, device="cuda")
    ld = torch.tensor([4, 4], dtype=torch.int32).cuda()
    mom, part = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda")
    call = lambda **kw: lib.fwn_actnorm_moments_ragged(*[kw.get(k, v) for k, v in (
        ("xa", buf.data_ptr()), ("xb", buf.data_ptr()), ("B", 2), ("rows", 4), ("Ch", 2), ("len", ld.data_ptr()), ("spr", 4),
        ("mom", mom.data_ptr()), ("scratch", part.data_ptr()), ("nbytes", 128), ("stream", None))])
    assert call(nbytes=lib.fwn_actnorm_moments_ragged_scratch_bytes(2, 4, 2)) == 0
    for bad in (dict(len=None), dict(Ch=3), dict(nbytes=8), dict(rows=0), dict(spr=0), dict(scratch=None), dict(xa=buf.data_ptr() + 2)):
        assert call(**bad) == -1 and b"fwn_actnorm_moments_ragged" in lib.fwn_last_error(), bad
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(2, 4, 3) == 0 and lib.fwn_actnorm_moments_ragged_scratch_bytes(0, 4, 2) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the whole model against the fp64 composition
@pytest.mark.parametrize("k", range(len(SMALL)))
def test_tables_and_clips_equal_the_fp64_composition(k):
    hp, t, lengths, x, c = _case(k)
    unit = int(np.lcm(hp.hop_size, 1 << hp.n_block))
    assert t in lengths and unit in lengths                                   # T itself and the shortest legal clip
    p64, lp0, ld0, z0 = _oracle(k)
    model = _fresh(hp, init=bool(k & 1))                                      # whatever init= the constructor got
    lp, ld, zp = model.forward_init(dev(x), dev(c), lengths, return_z=True)
    assert model._init is False
    assert lp.shape == ld.shape == (len(lengths),) and zp.shape == (2, len(lengths), t // 2)
    an = model.export_actnorm()
    first = "Block_0/Flow_0/ActNorm/"
    # not vacuous: the same composition with the count taken as all B x rows rows misses the first flow's logs by a multiple
    # of the bound (a wrong count shifts every flow's logs by log(valid fraction) / 6)
    wrong = oracle_ragged_init(W.synthetic_params(hp, 99, actnorm="zeros"), x, c, lengths, hp, count_all_rows_of=t, first_flow_only=True)
    off = float(np.abs(np.ravel(wrong[first + "logs"]) - np.ravel(p64[first + "logs"])).max())
    print("count = all B x rows rows: %slogs off by %.4f = %.1f x the bound" % (first, off, off / ABS_LOGS))
    assert off >= 10 * ABS_LOGS, off
    check_tables(an, p64, hp, "case %d" % k)
    np.testing.assert_allclose(np.ravel(an[first + "b"]), np.ravel(p64[first + "b"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.ravel(an[first + "logs"]), np.ravel(p64[first + "logs"]), rtol=1e-5, atol=1e-6)
    z = z_planes_to_squeezed(zp, hp.n_block, hp.n_flow).cpu().numpy()
    for b, n in enumerate(lengths):
        rows = n >> hp.n_block
        err = float(np.abs(z[b:b + 1, :rows] - z0[b]).max())
        print("clip %d (%d of %d samples): z max err %.3e, bound %.3e" % (b, n, t, err, ABS_Z))
        check_scalars(lp[b], ld[b], lp0[b], ld0[b])
        assert err <= ABS_Z, (k, b, n, err)
        assert not z[b, rows:].any()
    assert not _planes_past_the_end(zp, lengths).any()                        # exactly 0 past each clip


# ------------------------------------------------------------------ 3. padding is inert, bit for bit
def _tables(model):
    return {key: v.clone() for key, v in model._packed.an.items()}


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_padding_is_inert_bit_for_bit(k):
    hp, t, lengths, _, _ = _case(k)
    runs = []
    for junk in (False, True, True):                                          # zeros, junk, and a fresh model given the junk call again
        _, _, _, x, c = _case(k, junk)
        xd, cd = dev(x), dev(c)
        keep = (xd.clone(), cd.clone())
        model = _fresh(hp)
        out = model.forward_init(xd, cd, lengths, return_z=True)
        assert torch.equal(xd, keep[0]) and torch.equal(cd, keep[1])          # the caller's x and c are never written
        assert all(torch.isfinite(v).all() for v in out)
        runs.append((_tables(model), out))
    for tabs, out in runs[1:]:
        assert set(tabs) == set(runs[0][0])
        for key in tabs:
            assert torch.equal(tabs[key], runs[0][0][key]), key
        for a, b in zip(out, runs[0][1]):
            assert torch.equal(a, b)
    assert not _planes_past_the_end(runs[0][1][2], lengths).any()
    lp, ld = _fresh(hp).forward_init(dev(x), dev(c), np.asarray(lengths))      # lengths as an array, no return_z
    assert torch.equal(lp, runs[0][1][0]) and torch.equal(ld, runs[0][1][1])


# ------------------------------------------------------------------ 4. consistency
@pytest.mark.parametrize("k", range(len(SMALL)))
def test_forward_after_the_init_reproduces_its_scalars(k):
    """``forward(x, c, lengths=)`` right after ``forward_init`` runs the same stages on the same tables in the same order (the
    init pass only adds the moments and the table launch in front of each flow): bit-exact, asserted as such."""
    hp, t, lengths, x, c = _case(k)
    model = _fresh(hp)
    first = model.forward_init(dev(x), dev(c), lengths, return_z=True)
    tabs = _tables(model)
    again = model.forward(dev(x), dev(c), return_z=True, lengths=lengths)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for key, v in _tables(model).items():
        assert torch.equal(v, tabs[key])                                      # a forward leaves the tables alone


def test_equal_lengths_agree_with_the_plain_init():
    hp, t, lengths, x, c = _case(0)
    b = len(lengths)
    for n in (96, t):                                                         # all lengths L < T: the batch cropped to L; all T: the plain init
        ragged = _fresh(hp)
        ragged.forward_init(dev(x), dev(c), [n] * b)
        plain = _fresh(hp, init=True)
        plain.forward(dev(x[:, :n]), dev(c[:, :n // hp.hop_size]))
        check_tables(ragged.export_actnorm(), plain.export_actnorm(), hp, "all lengths %d of %d" % (n, t))


def test_first_flow_whitens_the_valid_rows():
    """Known answer: ActNorm of the clips' own rows with the exported Block_0/Flow_0 tables, in fp64 on the host, has mean 0 and
    mean square 1 per channel."""
    hp, t, lengths, x, c = _case(0)
    model = _fresh(hp)
    model.forward_init(dev(x), dev(c), lengths)
    an = model.export_actnorm()
    b_, logs = np.ravel(an["Block_0/Flow_0/ActNorm/b"]).astype(np.float64), np.ravel(an["Block_0/Flow_0/ActNorm/logs"]).astype(np.float64)
    rows = np.concatenate([onp.squeeze(x[k:k + 1, :n].astype(np.float64))[0] for k, n in enumerate(lengths)], axis=0)       # [rows][2]
    y = (rows + b_) * np.exp(3.0 * logs)
    np.testing.assert_allclose(y.mean(0), 0.0, atol=1e-5)
    np.testing.assert_allclose((y * y).mean(0), 1.0, atol=1e-4)


# ------------------------------------------------------------------ 5. refusals and entry points
def test_refusals():
    hp = small_hparams()
    params = W.synthetic_params(hp, 99, actnorm="zeros")
    model = FloWaveNet(hp).load_params(params)
    inp = W.synthetic_inputs(hp, 3, 64, want=("x", "c"))
    x, c = dev(inp["x"]), dev(inp["c"])
    for bad in BAD_LENGTHS:
        with pytest.raises(ValueError):
            model.forward_init(x, c, bad)
    lp, ld = model.forward_init(x, c, [64, 16, 48])
    assert lp.shape == ld.shape == (3,)
    fp8 = FloWaveNet(hp, gate_fp8=True).load_params(params)
    with pytest.raises(ValueError, match="gate_fp8"):
        fp8.forward_init(x, c, [64, 16, 48])
    with pytest.raises(ValueError, match="init"):                             # forward(lengths=) on an init=True model keeps raising
        FloWaveNet(hp, init=True).load_params(params).forward(x, c, lengths=[64, 16, 48])
    lib = _lib.load()
    ld_ = torch.tensor([64, 16, 48], dtype=torch.int32).cuda()
    out = torch.empty(2, 3, device="cuda")
    x32, c32 = x.float().contiguous(), c.float().contiguous()
    n = lib.fwn_ragged_init_workspace_bytes(C.byref(model._packed.model_desc), 3, 64)
    assert n >= lib.fwn_ragged_forward_workspace_bytes(C.byref(model._packed.model_desc), 3, 64) > 0
    assert lib.fwn_ragged_init_workspace_bytes(C.byref(fp8._packed.model_desc), 3, 64) == 0
    assert lib.fwn_ragged_init_workspace_bytes(C.byref(_lib.ModelDesc()), 3, 64) == 0
    assert lib.fwn_ragged_init_workspace_bytes(C.byref(model._packed.model_desc), 3, 60) == 0
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
    before = _tables(model)
    for m, lens, word in ((fp8, ld_.data_ptr(), b"fp8"), (model, None, b"null lengths")):
        rc = lib.fwn_model_forward_init_ragged(C.byref(m._packed.model_desc), 3, 64, x32.data_ptr(), c32.data_ptr(), lens, wsp, n,
                                               out.data_ptr(), None, None, None, None)
        assert rc == -1 and word in lib.fwn_last_error(), lib.fwn_last_error()
    rc = lib.fwn_model_forward_init_ragged(C.byref(model._packed.model_desc), 3, 64, x32.data_ptr(), c32.data_ptr(), ld_.data_ptr(), wsp,
                                           n - 1, out.data_ptr(), None, None, None, None)
    assert rc == -3 and b"workspace" in lib.fwn_last_error()
    torch.cuda.synchronize()
    for key, v in _tables(model).items():
        assert torch.equal(v, before[key])                                    # nothing ran


def test_trainer_ddi_with_lengths_then_a_step():
    hp, t, lengths, x, c = _case(0)
    params = W.synthetic_params(hp, 99, actnorm="zeros")
    tr = Trainer(hp, params, graph=False)
    tr.ddi(dev(x).reshape(len(lengths), t), dev(c), lengths=lengths)
    want = _fresh(hp, cond_mode=1, group=False)                               # Trainer.ddi's model: conditioning fused
    want.forward_init(dev(x), dev(c), lengths)
    views = tr.opt.master_views()
    for key, v in want.export_actnorm().items():
        assert np.array_equal(views[key].cpu().numpy().ravel(), np.ravel(v)), key
        assert float(views[key].abs().max()) > 0.0
    out = tr.step(dev(x).reshape(len(lengths), t), dev(c), lengths=lengths)
    assert all(math.isfinite(float(v)) for v in out)


DP_CFG = dict(n_block=4, n_flow=2, n_layer=3, hop_size=32, upsample_scales=[4, 8], num_mels=16)
DP_LENGTHS = [512, 32, 288, 160]


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)             # gloo moves CUDA tensors through the host; both ranks share cuda:0
    torch.cuda.set_device(0)
    hp = small_hparams(**DP_CFG)
    x, c = _ragged_inputs(hp, 4, 512, DP_LENGTHS, True)
    lo = 2 * rank
    tr = Trainer(hp, W.synthetic_params(hp, 11, actnorm="zeros"), graph=False)
    tr.ddi(dev(x[lo:lo + 2]).reshape(2, 512), dev(c[lo:lo + 2]), lengths=DP_LENGTHS[lo:lo + 2])
    views = tr.opt.master_views()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **{k: v.cpu().numpy() for k, v in views.items() if "/ActNorm/" in k})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ragged_init_matches_one_process_on_the_whole_batch(tmp_path):
    """Two gloo ranks, two clips each - 544 and 448 samples, so the ranks hold different numbers of rows: the all-reduced row
    count weights them, both ranks end with identical tables, within the table bounds of the one-process init on the four
    clips."""
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
    r0, r1 = (dict(np.load(tmp_path / ("rank%d.npz" % r))) for r in range(2))
    assert set(r0) == set(r1) and len(r0) == 2 * DP_CFG["n_block"] * DP_CFG["n_flow"]
    for key in r0:
        assert np.array_equal(r0[key], r1[key]), key
    hp = small_hparams(**DP_CFG)
    x, c = _ragged_inputs(hp, 4, 512, DP_LENGTHS, True)
    one = FloWaveNet(hp, group=False).load_params(W.synthetic_params(hp, 11, actnorm="zeros"))
    one.forward_init(dev(x), dev(c), DP_LENGTHS)
    check_tables(r0, one.export_actnorm(), hp, "two ranks against one process")


# ------------------------------------------------------------------ 6. train.py --ragged
def _train_args(tmp_path, **kw):
    from types import SimpleNamespace
    return SimpleNamespace(base_dir=str(tmp_path), restore=False, summary_interval=2, checkpoint_interval=3, eval_interval=1000,
                           train_steps=3, seed=3, ragged=True, **kw)


def test_train_cli_on_a_corpus_of_short_utterances_only(tmp_path):
    """No utterance is longer than max_time_steps: ``next_full`` has nothing to draw from (before the ragged init this run
    raised ``ValueError`` at step 0).  The init takes a ragged batch, the init-step update runs with its lengths, the run
    goes on to its last step and writes the checkpoint."""
    import json
    from test_ragged_train_host import _write
    from tf_flowavenet_amd import train as TL
    hp, path, _ = _write(tmp_path, "abe")
    with pytest.raises(ValueError, match="init=True takes no lengths"):
        TL.Dataset(path, hp, seed=3, ragged=True).next_full()
    log_dir = str(tmp_path / "logs")
    save_dir = TL.train(log_dir, _train_args(tmp_path), hp, "train.txt")
    assert "flowavenet_model.ckpt-3.npz" in os.listdir(save_dir)
    recs = [json.loads(line) for line in open(os.path.join(log_dir, "train", "summary.jsonl"))]
    assert [r["step"] for r in recs] == [2] and np.isfinite(recs[0]["losses/total_loss"]) and recs[0]["mean_clip_length"] < 256
    ck = np.load(os.path.join(save_dir, "flowavenet_model.ckpt-3.npz"))
    assert all(np.isfinite(ck[k]).all() for k in ck.files)
    assert float(np.abs(ck["Block_0/Flow_0/ActNorm/b"]).max()) > 0.0          # the init ran


def test_train_cli_init_batch_on_a_corpus_with_a_long_utterance(tmp_path, monkeypatch):
    """Default: the init batch is ``next_full``'s for the same seed, without lengths, as before.  ``--ragged_init``: a batch
    drawn as ``next_train`` draws, with its lengths."""
    from test_ragged_train_host import _write
    from tf_flowavenet_amd import train as TL
    hp, path, _ = _write(tmp_path, "abcde")
    seen = []
    real = Trainer.ddi

    def spy(self, x, c, lengths=None):
        seen.append((np.array(x), np.array(c), None if lengths is None else np.array(lengths)))
        return real(self, x, c, lengths=lengths)

    monkeypatch.setattr(Trainer, "ddi", spy)
    for k, flag in enumerate((False, True)):
        args = _train_args(tmp_path, ragged_init=flag)
        args.train_steps = 1                                                  # the init step is the run
        TL.train(str(tmp_path / ("logs%d" % k)), args, hp, "train.txt")
    ds = TL.Dataset(path, hp, seed=3, ragged=True)
    mels, audios = ds.next_full()
    assert seen[0][2] is None and np.array_equal(seen[0][0], audios) and np.array_equal(seen[0][1], mels)
    mels, audios, lens = TL.Dataset(path, hp, seed=3, ragged=True).next_init()
    assert np.array_equal(seen[1][2], lens) and np.array_equal(seen[1][0], audios) and np.array_equal(seen[1][1], mels)
    assert lens.min() < 256                                                   # seed 3 draws short utterances into it
