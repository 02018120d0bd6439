"""Gradient accumulation (-m gpu): ``fwn_grad_accumulate`` bit for bit, and ``Trainer.accumulate`` / ``Trainer.step`` - one
optimiser update over K micro-batches whose gradients are summed in call order and averaged by the loss scale K.

Bounds: the kernel and every statement about the sum, its order, the recorded step, ``repack=False`` and the two ranks'
lock-step are exact (bit patterns).  The oracle comparisons take tests/test_train.py's per-tensor rule (``grad_rel_allowed``,
median 3e-2, cosine > 0.999) and tests/test_ragged_train.py's (the same rule, ``MEDIAN``) by import; the two-rank gradient
takes the cosine and norm bounds of ``test_two_rank_data_parallel_step_matches_one_process_on_the_whole_batch``."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import small_hparams
from test_train import grad_rel_allowed
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import training as TR
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.training import GradEngine, Trainer

pytestmark = pytest.mark.gpu

CFG = dict(n_block=3, n_flow=2, n_layer=2, hop_size=16, upsample_scales=[4, 4], num_mels=16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. the kernel
def _big_n():
    """More than two sweeps of the launcher's grid plus a ragged tail.  The launcher takes ``fwn_sqnorm_blocks`` workgroups
    (what ``fwn_grad_norm_partials`` reports) of 256 lanes x 4 elements; a huge n reads the cap itself."""
    cap = int(_lib.load().fwn_grad_norm_partials(1 << 40))
    return 2 * cap * 1024 + 5 * 1024 + 3


SIZES = (1, 3, 4, 5, 7, 1023, 1024, 1025, "big")
OFFSETS = ((0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 2), (2, 0, 0))
# (a, b): signed zeros, infinities, NaN on either side, inf - inf, pairs that overflow, exact cancellation, a lost addend and
# the two roundings next to it
_POOL = np.array([(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (np.inf, 1.0), (-np.inf, 5.0), (np.inf, -np.inf), (np.nan, 1.0),
                  (1.0, np.nan), (3e38, 3e38), (-3e38, -3e38), (2e38, 1.5e38), (1.5, -1.5), (1e-30, 1e30), (1.0, 2.0 ** -24),
                  (1.0, 2.0 ** -23), (1.0, 3 * 2.0 ** -25), (-np.inf, -np.inf)], dtype=np.float32)
_VALUES = {}


def _values(n):
    """(a, b, a + b in NumPy fp32) for one size, computed once.  Normal numbers over a wide range of exponents; the special
    pairs fill the front (rotated by n, so the tiny sizes see different ones) and, for the long sizes, the very end."""
    if n not in _VALUES:
        rng = np.random.default_rng(n)
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)).astype(np.float32)
        b = (rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)).astype(np.float32)
        k = min(n, len(_POOL))
        pick = (np.arange(k) + n) % len(_POOL)
        a[:k], b[:k] = _POOL[pick, 0], _POOL[pick, 1]
        if n > 2 * len(_POOL):
            a[-len(_POOL):], b[-len(_POOL):] = _POOL[:, 0], _POOL[:, 1]
        tiny = np.float32(2.0 ** -126)
        assert not ((a != 0) & (np.abs(a) < tiny)).any() and not ((b != 0) & (np.abs(b) < tiny)).any()      # no subnormal inputs
        with np.errstate(over="ignore", invalid="ignore"):
            _VALUES[n] = (a, b, a + b)
    return _VALUES[n]


SENTINEL = 12345.678


@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_numpy_fp32_bit_for_bit(size, offsets):
    """dst = a + b against NumPy's fp32 ``a + b`` by bit pattern, NaN as a mask.  Subnormals: the inputs hold none, and an
    element whose reference SUM is subnormal (non-zero, below 2^-126) is left out of the bit comparison.  Every buffer is
    sentinel-filled and dst sits four floats in: whatever lies outside dst[0, n) - the four sentinels before and after it and
    the rest - must be untouched, and so must the sources."""
    lib = _lib.load()
    n = _big_n() if size == "big" else size
    a_np, b_np, ref = _values(n)
    normal = ~((ref != 0) & (np.abs(ref) < np.float32(2.0 ** -126)))
    a_t, b_t = dev(a_np), dev(b_np)
    st = torch.cuda.current_stream().cuda_stream

    def buf(off, fill=None):
        t = torch.full((4 + off + n + 4 + 3,), SENTINEL, dtype=torch.float32, device="cuda")
        if fill is not None:
            t[4 + off:4 + off + n] = fill
        return t

    for mode in ("null", "dst_is_a", "dst_is_b", "distinct"):
        od, oa, ob = offsets
        if mode == "dst_is_a":
            oa = od
        if mode == "dst_is_b":
            ob = od
        D = buf(od, a_t if mode == "dst_is_a" else b_t if mode == "dst_is_b" else None)
        A = D if mode == "dst_is_a" else None if mode == "null" else buf(oa, a_t)
        B = D if mode == "dst_is_b" else buf(ob, b_t)
        keep_a = A.clone() if A is not None and A is not D else None
        keep_b = B.clone() if B is not D else None
        ptr = lambda t, o: t.data_ptr() + 4 * (4 + o)
        rc = lib.fwn_grad_accumulate(ptr(D, od), ptr(A, oa) if A is not None else None, ptr(B, ob), n, st)
        _lib.check(rc, "fwn_grad_accumulate")
        torch.cuda.synchronize()
        got = D[4 + od:4 + od + n].cpu().numpy()
        want = b_np if mode == "null" else ref
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (mode, n, offsets)
        cmp = ~nan & (normal if mode != "null" else True)
        assert np.array_equal(got.view(np.uint32)[cmp], want.view(np.uint32)[cmp]), (mode, n, offsets)
        outside = torch.cat([D[:4 + od], D[4 + od + n:]])
        assert bool((outside == SENTINEL).all()), (mode, n, offsets)
        if keep_a is not None:
            assert torch.equal(A.view(torch.int32), keep_a.view(torch.int32)), (mode, n, offsets)
        if keep_b is not None:
            assert torch.equal(B.view(torch.int32), keep_b.view(torch.int32)), (mode, n, offsets)


# ------------------------------------------------------------------ trainers on small batches
def _hp():
    return small_hparams(**CFG)


_INP = {}


def _batch(k, b=2, t=256):
    """Micro-batch k: b clips of T = t out of the four synthetic ones, rolled and scaled so that every k differs."""
    hp = _hp()
    if "x" not in _INP:
        inp = W.synthetic_inputs(hp, 4, 256)
        _INP["x"], _INP["c"] = dev(inp["x"]).reshape(4, 256), dev(inp["c"])
    x, c = _INP["x"].roll(k, 0) * (1.0 - 0.05 * (k % 7)), _INP["c"].roll(k, 0)
    return x[:b, :t].contiguous(), c[:b, :t // hp.hop_size].contiguous()


def _flat_grad(eng, opt, x, c, **kw):
    """``engine.loss_and_grads`` on the optimiser's masters into a flat buffer of its own -> (scalars, flat gradient)."""
    flat = torch.zeros_like(opt.g)
    out = eng.loss_and_grads(opt.master_views(), x, c, grad_out=opt.layout.views(flat), **kw)
    torch.cuda.synchronize()
    return torch.stack(out[:3]).clone(), flat


# ------------------------------------------------------------------ 2. the sum and its order
def test_three_micro_batches_sum_in_call_order_and_update_once():
    hp = _hp()
    tr = Trainer(hp, W.synthetic_params(hp, 11), graph=False)
    tr.ddi(*_batch(0, 4))
    assert tr.opt.acc is None and tr.pending == 0
    w0 = tr.opt.w.clone()
    eng = GradEngine(hp)
    parts = [_flat_grad(eng, tr.opt, *_batch(k)) for k in range(3)]
    want = (parts[0][1] + parts[1][1]) + parts[2][1]
    outs = []
    for k in range(2):
        outs.append(torch.stack(tr.accumulate(*_batch(k))))
        assert tr.pending == k + 1 and tr.opt.global_step == 0 and torch.equal(tr.opt.w, w0)
        assert torch.equal(outs[-1], parts[k][0])                    # each call returns its own micro-batch's scalars
    loss, log_p, logdet, gnorm = tr.step(*_batch(2))
    torch.cuda.synchronize()
    assert tr.pending == 0 and tr.opt.global_step == 1
    assert torch.equal(tr.opt.g, want)
    assert torch.equal(torch.stack([loss, log_p, logdet]), ((parts[0][0] + parts[1][0]) + parts[2][0]) / 3.0)
    # the update: a second trainer on the same masters whose gradient buffer is set to that sum, stepped with loss scale 3
    tr2 = Trainer(hp, W.synthetic_params(hp, 11), graph=False)
    tr2.opt.w.copy_(w0)
    tr2.opt.g.copy_(want)
    gnorm2 = tr2.opt.step(loss_scale=3)
    torch.cuda.synchronize()
    for name in ("w", "m", "v"):
        assert torch.equal(getattr(tr.opt, name), getattr(tr2.opt, name)), name
    assert torch.equal(gnorm, gnorm2) and float(gnorm) > 0 and not torch.equal(tr.opt.w, w0)


# ------------------------------------------------------------------ 3. against the fp64 oracle
def _check_against_oracle(g, g0, hp, median):
    """tests/test_train.py's per-tensor rule (``test_loss_and_all_parameter_gradients_match_autograd_oracle``)."""
    assert sorted(g) == sorted(g0)
    total = float(np.sqrt(sum(float((np.asarray(v) ** 2).sum()) for v in g0.values())))
    rels, dot, na, nb_ = [], 0.0, 0.0, 0.0
    for k in sorted(g0):
        a, r = g[k].cpu().numpy().astype(np.float64).reshape(-1), np.asarray(g0[k], dtype=np.float64).reshape(-1)
        if "res_conv" in k and ("ResBlock_%d/" % (hp.n_layer - 1)) in k:
            assert not a.any() and not r.any(), k          # dead conv: zero gradient, and 0 + 0 stays 0
            continue
        nr = np.linalg.norm(r)
        rel = np.linalg.norm(a - r) / nr
        rels.append(rel)
        assert rel < grad_rel_allowed(nr, total, rel), (k, rel, nr, total)
        dot += float(a @ r); na += float(a @ a); nb_ += float(r @ r)
    print("median relative error %.4f, worst %.4f, cosine %.6f" % (np.median(rels), max(rels), dot / np.sqrt(na * nb_)))
    assert np.median(rels) < median, np.median(rels)
    assert dot / np.sqrt(na * nb_) > 0.999


def test_two_micro_batches_of_two_clips_match_the_oracle_on_the_four_clips():
    from oracle import grad_torch as G
    hp = _hp()
    p = W.synthetic_params(hp, 5)
    inp = W.synthetic_inputs(hp, 4, 256)
    loss0, lp0, ld0, g0 = G.loss_and_grads(p, inp["x"], inp["c"], hp)
    x, c = dev(inp["x"]).reshape(4, 256), dev(inp["c"])
    tr = Trainer(hp, p, graph=False)
    tr.accumulate(x[:2], c[:2])
    loss, lp, ld, _ = tr.step(x[2:], c[2:])
    torch.cuda.synchronize()
    assert abs(float(lp) - lp0) < 1e-3 * abs(lp0) and abs(float(ld) - ld0) < 1e-3 * max(1.0, abs(ld0))
    _check_against_oracle({k: v / 2 for k, v in tr.opt.grad_views().items()}, g0, hp, 3e-2)


def test_two_ragged_micro_batches_match_the_mean_of_the_per_clip_oracle_gradients():
    """Case A of tests/test_ragged_train.py (T = 128, lengths 128, 16, 64, 96; its parameters, its oracle - computed once and
    shared with that file - and its bounds), split into two micro-batches of two clips."""
    import test_ragged_train as R
    hp, t, lengths, x, c = R._case("A")
    per, g0 = R._oracle("A")
    tr = Trainer(hp, R._params(hp), graph=False)
    xd, cd = dev(x).reshape(4, t), dev(c)
    tr.accumulate(xd[:2], cd[:2], lengths=lengths[:2])
    assert tr.per_clip[0].shape == (2,)
    loss, lp, ld, _ = tr.step(xd[2:], cd[2:], lengths=lengths[2:])
    torch.cuda.synchronize()
    lp0, ld0 = (float(np.mean([v[i] for v in per])) for i in (1, 2))
    assert abs(float(lp) - lp0) <= R.REL_LOGP * abs(lp0) and abs(float(ld) - ld0) <= R.ABS_LOGDET * max(1.0, abs(ld0))
    _check_against_oracle({k: v / 2 for k, v in tr.opt.grad_views().items()}, g0, hp, R.MEDIAN["A"])


# ------------------------------------------------------------------ 4. repack=False
def test_skipping_the_repack_on_unchanged_masters_gives_the_same_bits(monkeypatch):
    hp = _hp()
    tr = Trainer(hp, W.synthetic_params(hp, 11), graph=False)
    tr.ddi(*_batch(0, 4))
    calls = []
    refresh = TR._TrainPack.refresh
    monkeypatch.setattr(TR._TrainPack, "refresh", lambda self: (calls.append(1), refresh(self))[1])
    eng = GradEngine(hp)
    s0, g0 = _flat_grad(eng, tr.opt, *_batch(0))                 # the first call packs (the plan is built)
    s1, g1 = _flat_grad(eng, tr.opt, *_batch(0))
    assert len(calls) == 1
    s2, g2 = _flat_grad(eng, tr.opt, *_batch(0), repack=False)
    s3, g3 = _flat_grad(eng, tr.opt, *_batch(1), repack=False)
    assert len(calls) == 1                                       # ... and repack=False really skipped it
    fresh = _flat_grad(GradEngine(hp), tr.opt, *_batch(1))
    assert torch.equal(g1, g0) and torch.equal(g2, g0) and torch.equal(s2, s0)
    assert torch.equal(g3, fresh[1]) and torch.equal(s3, fresh[0]) and bool(g0.any())


# ------------------------------------------------------------------ 5. recorded equals eager
def test_recorded_updates_equal_eager_updates_bit_for_bit():
    """K changes between updates (2, 1, 3), every batch differs, each round ends with a ragged update, and a second input
    shape comes in between - after the first shape's recordings exist, which must stay valid.  Three visits take a recording
    from its eager warm-up through the capture to a replay: every kind (first / later micro-batch, final step with 1 and 2
    pending, the plain step) gets there."""
    hp = _hp()
    lens = ([256, 96], [16, 256], [160, 48], [256, 256], [64, 16], [208, 112])
    updates = []
    for rnd in range(3):
        if rnd == 2:
            updates += [("half", 2, None)] * 3
        updates += [("full", 2, None), ("full", 1, None), ("full", 3, None), ("full", 2, lens[2 * rnd:2 * rnd + 2])]
    runs = {}
    for graph in (False, True):
        tr = Trainer(hp, W.synthetic_params(hp, 11), graph=graph)
        tr.ddi(*_batch(0, 4))
        outs, k, w_mid = [], 0, None
        for shape, K, ragged in updates:
            for micro in range(K):
                x, c = _batch(k, 2, 256 if shape == "full" else 128)
                k += 1
                call = tr.step if micro == K - 1 else tr.accumulate
                out = call(x, c, lengths=ragged[micro]) if ragged else call(x, c)
                outs.append(tuple(float(v) for v in out))
                if ragged:
                    outs.append(tuple(tr.per_clip[0].tolist()) + tuple(tr.per_clip[1].tolist()))
                else:
                    assert tr.per_clip is None
            if len(outs) == 10:
                w_mid = tr.opt.w.clone()
        assert tr.graph is graph and tr.pending == 0             # the recording did not fall back to eager steps
        runs[graph] = (outs, w_mid, tr.opt.w.clone(), tr.opt.global_step)
        if graph:
            kinds = sorted((key[0][0][1], key[0][-1] == "ragged") + key[1] for key, v in tr._recorded_acc.items() if isinstance(v, dict))
            full = [kd[2:] for kd in kinds if kd[0] == 256 and not kd[1]]
            assert full == [("micro", False), ("micro", True), ("step", 1), ("step", 2)], kinds
            assert [kd[2:] for kd in kinds if kd[1]] == [("micro", True), ("step", 1)], kinds
            assert [kd[2:] for kd in kinds if kd[0] == 128] == [("micro", True), ("step", 1)], kinds
            assert all(isinstance(v, dict) for v in tr._recorded_acc.values())
    assert runs[True][3] == runs[False][3] == len(updates)
    assert all(np.isfinite(v) for o in runs[True][0] for v in o)
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1]) and torch.equal(runs[True][2], runs[False][2])


# ------------------------------------------------------------------ 6. the plain path
def test_plain_steps_allocate_no_accumulator_and_make_no_new_recording():
    hp = _hp()
    tr = Trainer(hp, W.synthetic_params(hp, 11))
    tr.ddi(*_batch(0, 4))
    for k in range(3):
        tr.step(*_batch(k))
    torch.cuda.synchronize()
    assert tr.opt.acc is None and tr.pending == 0 and tr._recorded_acc == {} and len(tr._recorded) == 1


# ------------------------------------------------------------------ 7. two ranks
def _dp_accum_worker(rank, world, port, out_dir, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)      # gloo moves CUDA tensors through the host; both ranks share cuda:0
    torch.cuda.set_device(0)
    hp = _hp()
    inp = W.synthetic_inputs(hp, 4, 256)
    x = torch.from_numpy(inp["x"]).reshape(4, 256)[2 * rank:2 * rank + 2].cuda()
    c = torch.from_numpy(inp["c"])[2 * rank:2 * rank + 2].cuda()
    tr = Trainer(hp, W.synthetic_params(hp, 11), graph=graph)
    tr.ddi(x, c)
    w0 = tr.opt.w.clone()
    keep = {}
    for u in range(3):              # with graph=True: eager, recorded, replayed
        tr.accumulate(x[:1], c[:1])
        tr.step(x[1:], c[1:])
        if u == 0:
            keep = dict(g=tr.opt.g.cpu().numpy(), w1=tr.opt.w.cpu().numpy())
    assert tr.graph is graph and tr.opt.global_step == 3
    if graph:       # the micro-batch is ONE graph at world 2, the final step a chain cut at every range
        assert len(tr._recorded_acc[next(k for k in tr._recorded_acc if k[1] == ("micro", True))]["segs"]) == 1
        assert len(tr._recorded_acc[next(k for k in tr._recorded_acc if k[1] == ("step", 1))]["segs"]) == hp.n_block + 2
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), w0=w0.cpu().numpy(), g3=tr.opt.g.cpu().numpy(), w3=tr.opt.w.cpu().numpy(), **keep)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_in_lock_step_and_sum_the_four_clips(tmp_path):
    """Two processes (gloo, both on cuda:0), K = 2, one clip per micro-batch per rank: the ranks end every update with
    bit-identical gradients and weights, recorded and eager alike, and the all-reduced sum of the four one-clip gradients is
    4 x the gradient of the four-clip batch in one process (the two-rank test's bounds: cosine > 0.999, norms within 2 %)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")

    def run_pair(out, graph):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()      # a fresh port per pair
        procs = [ctx.Process(target=_dp_accum_worker, args=(r, 2, port, str(out), graph), daemon=True) for r in range(2)]
        for p in procs:
            p.start()
        try:
            for p in procs:
                p.join(timeout=150)
            return [p.exitcode for p in procs]
        finally:
            for p in procs:         # a rank that died leaves its peer waiting in a collective: never leave it behind
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)

    res = {}
    for graph in (True, False):
        out = tmp_path / ("graph%d" % graph)
        out.mkdir()
        assert run_pair(out, graph) == [0, 0]
        r0, r1 = (np.load(out / ("rank%d.npz" % r)) for r in range(2))
        for name in ("w0", "g", "w1", "g3", "w3"):
            assert np.array_equal(r0[name], r1[name]), (graph, name)
        res[graph] = r0
    for name in ("g", "w1", "g3", "w3"):
        assert np.array_equal(res[True][name], res[False][name]), name
    hp = _hp()
    inp = W.synthetic_inputs(hp, 4, 256)
    tr = Trainer(hp, W.synthetic_params(hp, 11), graph=False)
    tr.opt.w.copy_(torch.from_numpy(res[True]["w0"]))
    _, flat = _flat_grad(tr.engine, tr.opt, dev(inp["x"]).reshape(4, 256), dev(inp["c"]))
    want, got = 4.0 * flat.cpu().numpy().astype(np.float64), res[True]["g"].astype(np.float64)
    cos = float((want * got).sum() / np.sqrt((want * want).sum() * (got * got).sum()))
    assert cos > 0.999 and abs(np.linalg.norm(got) / np.linalg.norm(want) - 1.0) < 2e-2, (cos, np.linalg.norm(got), np.linalg.norm(want))


# ------------------------------------------------------------------ 8. refusals, drop_pending, the sharded exchange
@pytest.mark.parametrize("graph", [False, True])
def test_another_batch_size_is_refused_and_drop_pending_gives_back_the_plain_step(graph):
    hp = _hp()
    ref = Trainer(hp, W.synthetic_params(hp, 11), graph=graph)
    ref.ddi(*_batch(0, 4))
    want = tuple(float(v) for v in ref.step(*_batch(3)))
    tr = Trainer(hp, W.synthetic_params(hp, 11), graph=graph)
    tr.ddi(*_batch(0, 4))
    tr.accumulate(*_batch(1))
    acc = tr.opt.acc.clone()
    for call in (tr.accumulate, tr.step):
        with pytest.raises(ValueError, match="clips"):
            call(*_batch(2, 3))
        with pytest.raises(ValueError):                              # a bad length is refused on the host as well
            call(*_batch(2), lengths=[256, 24])
    torch.cuda.synchronize()
    assert tr.pending == 1 and tr.opt.global_step == 0 and torch.equal(tr.opt.acc, acc) and torch.equal(tr.opt.w, ref.opt.w) is False
    tr.accumulate(*_batch(2, 2, 128))                                # another T is fine
    assert tr.pending == 2
    tr.drop_pending()
    assert tr.pending == 0
    got = tuple(float(v) for v in tr.step(*_batch(3)))
    torch.cuda.synchronize()
    assert got == want and torch.equal(tr.opt.w, ref.opt.w) and torch.equal(tr.opt.g, ref.opt.g)


def test_the_sharded_exchange_folds_the_whole_buffer_and_matches_the_all_reduce_path_in_one_process():
    """exchange="zero1" is eager only; in one process its update is the all-reduce path's own, so the two trainers must agree
    bit for bit - the pending sum folded once over the whole buffer on one side, range by range on the other."""
    hp = _hp()
    res = []
    for exchange in ("allreduce", "zero1"):
        tr = Trainer(hp, W.synthetic_params(hp, 11), graph=True)
        tr.opt.exchange = exchange
        tr.ddi(*_batch(0, 4))
        tr.accumulate(*_batch(0))
        tr.accumulate(*_batch(1))
        out = tr.step(*_batch(2))
        torch.cuda.synchronize()
        assert (tr._recorded_acc == {}) == (exchange == "zero1")
        res.append((tuple(float(v) for v in out), tr.opt.g.clone(), tr.opt.w.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


# ------------------------------------------------------------------ 9. the CLI
def test_train_cli_accum_steps_counts_updates_and_consumes_the_draws_in_order(tmp_path, monkeypatch):
    """--accum_steps 2 on the tiny corpus of tests/test_train.py's CLI test: a few updates, a checkpoint, a resume.  The first
    run's draw 0 is the init step's (one batch, as ever); after it - and from draw 0 of the resumed run, whose Dataset is
    seeded afresh - update u takes draws 2u and 2u + 1: accumulate, then step."""
    import wave
    from types import SimpleNamespace
    from tf_flowavenet_amd import preprocessing as P, train as TL
    hp = small_hparams(n_fft=64, sample_rate=8000, fmin=50, fmax=3800, max_time_steps=256, batch_size=4, test_size=2,
                       eval_max_time_steps=512, **CFG)
    book = tmp_path / "raw" / "book"
    os.makedirs(book / "wavs")
    rng = np.random.default_rng(0)
    lines = []
    for i in range(6):
        n = 900 + 37 * i
        pcm = (np.clip(0.3 * rng.standard_normal(n), -1, 1) * 32767).astype("<i2")
        with wave.open(str(book / "wavs" / ("u%d.wav" % i)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(hp.sample_rate); w.writeframes(pcm.tobytes())
        lines.append("u%d|t|t" % i)
    (book / "metadata.csv").write_text("\n".join(lines), encoding="utf-8")
    data = tmp_path / "base" / "training_data"
    P.preprocess(str(tmp_path / "raw"), str(data), hp)
    calls = []
    for name in ("accumulate", "step"):
        def spy(self, x, c, lengths=None, _name=name, _real=getattr(Trainer, name)):
            calls.append((_name, np.array(x), self.opt.global_step))
            return _real(self, x, c, lengths)
        monkeypatch.setattr(Trainer, name, spy)
    # one summary, at the last update, and no evaluation: the test draws come after every training draw of a run
    args = SimpleNamespace(base_dir=str(tmp_path / "base"), restore=True, summary_interval=4, checkpoint_interval=2,
                           eval_interval=100, train_steps=4, seed=3, accum_steps=2)
    log_dir = str(tmp_path / "base" / "logs")
    save_dir = TL.train(log_dir, args, hp, "training_data/train.txt")
    shadow = TL.Dataset(str(data / "train.txt"), hp, seed=3)
    assert [(n, s) for n, _, s in calls] == [("step", 0)] + [("accumulate", 1), ("step", 1), ("accumulate", 2), ("step", 2), ("accumulate", 3), ("step", 3)]
    for n, x, _ in calls:
        assert np.array_equal(x, shadow.next_train()[1]), n
    ckpts = sorted(os.listdir(save_dir))
    assert ckpts == ["flowavenet_model.ckpt-2.npz", "flowavenet_model.ckpt-4.npz"]
    assert int(np.load(os.path.join(save_dir, ckpts[-1]))["__opt/global_step"]) == 4
    recs = [json.loads(l) for l in open(os.path.join(log_dir, "train", "summary.jsonl"))]
    assert [r["step"] for r in recs] == [4] and recs[0]["accum_steps"] == 2 and np.isfinite(recs[0]["losses/total_loss"])
    # resume: picks up at update 4 and runs to 6, no init step
    del calls[:]
    args.train_steps, args.summary_interval = 6, 6
    TL.train(log_dir, args, hp, "training_data/train.txt")
    shadow = TL.Dataset(str(data / "train.txt"), hp, seed=3)
    assert [(n, s) for n, _, s in calls] == [("accumulate", 4), ("step", 4), ("accumulate", 5), ("step", 5)]
    for u in range(2):
        assert np.array_equal(calls[2 * u][1], shadow.next_train()[1]) and np.array_equal(calls[2 * u + 1][1], shadow.next_train()[1])
    assert "flowavenet_model.ckpt-6.npz" in os.listdir(save_dir)
    recs = [json.loads(l) for l in open(os.path.join(log_dir, "train", "summary.jsonl"))]
    assert [r["step"] for r in recs] == [4, 6] and all(r["accum_steps"] == 2 for r in recs)
