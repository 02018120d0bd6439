"""Ragged forward (-m gpu): ``FloWaveNet.forward(x, c, lengths=)`` gives every clip of a batch the ``log_p`` and ``logdet``
that clip gets alone, whatever the batch holds past the clip's end.

Cases: those of tests/test_ragged.py (``SMALL``: each holds T itself and the shortest legal clip, one has a single row at the
last block, one a dilation of 27 that reaches past the short clips).  Tolerances: tests/test_gpu_parity.py's, copied - the
suite's bounds for bf16 hidden activations with fp32 accumulation; statements about the padding and repeated calls are exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams, hparams8000
from tf_flowavenet_amd.model import FloWaveNet, z_planes_to_squeezed

from conftest import small_hparams

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_LOGP = 1e-3
ABS_LOGDET = 1e-3
ABS_Z = 2e-2
ABS_WAV = 1e-2

SMALL = [
    (dict(), 256, [256, 16, 160, 96]),
    (dict(n_block=4, n_flow=2), 256, [160, 256, 16, 208]),
    (dict(n_block=2, n_flow=4, n_layer=4), 192, [192, 16, 64, 112]),                   # dilation 27 reaches past the short clips
    (dict(n_block=5, n_flow=2, num_mels=16, hop_size=32, upsample_scales=[4, 8]), 128, [32, 128, 64, 96]),   # one row at the last block
    ("8k", 480, [480, 96, 192, 384]),                                                    # hparams8000's geometry: hop 96 = 8 x 12, n_block 5
]
BAD_LENGTHS = ([64, 64], [64, 64, 64, 64], [64, 24, 64], [64, 80, 64], [64, 0, 64], [64, 8, 64], [64, -16, 64], [64, 32.5, 64], 64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_scalars(log_p, logdet, lp0, ld0):
    print("log_p %.6f (oracle %.6f)  logdet %.6f (oracle %.6f)" % (float(log_p), lp0, float(logdet), ld0))
    assert abs(float(log_p) - lp0) <= REL_LOGP * abs(lp0), (float(log_p), lp0)
    assert abs(float(logdet) - ld0) <= ABS_LOGDET * max(1.0, abs(ld0)), (float(logdet), ld0)


def _hp(cfg):
    return hparams8000().replace(n_flow=2, num_mels=16) if cfg == "8k" else small_hparams(**cfg)


def _ragged_inputs(hp, b, t, lengths, junk):
    """x, c of W.synthetic_inputs with the part past each clip's length replaced: zeros, or junk (x: 3 N(0,1), mel: 1.0)."""
    inp = W.synthetic_inputs(hp, b, t, want=("x", "c"))
    x, c = inp["x"].copy(), inp["c"].copy()
    rng = np.random.default_rng(5)
    for k, n in enumerate(lengths):
        x[k, n:] = 3.0 * rng.standard_normal(x[k, n:].shape) if junk else 0.0
        c[k, n // hp.hop_size:] = 1.0 if junk else 0.0
    return x.astype(np.float32), c.astype(np.float32)


def _planes_past_the_end(zp, lengths):
    """The part of the z planes [2][B][T/2] past each clip's end, as one tensor."""
    return torch.cat([zp[:, k, n // 2:].reshape(-1) for k, n in enumerate(lengths)])


@pytest.mark.parametrize("cfg,t,lengths", SMALL + [("full", 4096, [4096, 256, 2048, 3072])])
def test_padding_is_inert_bit_for_bit(cfg, t, lengths):
    hp = default_hparams() if cfg == "full" else _hp(cfg)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    outs = []
    for junk in (False, True):
        x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk)
        xd, cd = dev(x), dev(c)
        keep = (xd.clone(), cd.clone())
        outs.append(model.forward(xd, cd, return_z=True, lengths=lengths))
        assert torch.equal(xd, keep[0]) and torch.equal(cd, keep[1])          # the caller's x and c are never written
    for lp, ld, zp in outs:
        assert lp.shape == ld.shape == (len(lengths),) and lp.dtype == ld.dtype == torch.float32
        assert zp.shape == (2, len(lengths), t // 2)
        assert torch.isfinite(lp).all() and torch.isfinite(ld).all() and torch.isfinite(zp).all()
        assert not _planes_past_the_end(zp, lengths).any()                    # exactly 0 past each clip
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for k, n in enumerate(lengths):
        assert float(outs[1][2][:, k, :n // 2].abs().max()) > 0.0
    # lengths as a NumPy array, a CPU tensor and a device tensor are the same call; so is the same call again
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, True)
    for form in (np.asarray(lengths), torch.tensor(lengths), torch.tensor(lengths, dtype=torch.int32).cuda(), list(lengths)):
        for a, b in zip(model.forward(dev(x), dev(c), return_z=True, lengths=form), outs[1]):
            assert torch.equal(a, b)
    lp, ld = model.forward(dev(x), dev(c), lengths=lengths)                   # and without return_z
    assert torch.equal(lp, outs[1][0]) and torch.equal(ld, outs[1][1])


@pytest.mark.parametrize("cfg,t,lengths", SMALL)
def test_each_clip_equals_the_oracle_forward_of_that_clip_alone(cfg, t, lengths):
    hp = _hp(cfg)
    unit = int(np.lcm(hp.hop_size, 1 << hp.n_block))
    assert t in lengths and unit in lengths                                   # T itself and the shortest legal clip
    params = W.synthetic_params(hp, 99, actnorm="random")
    p64 = onp.to_f64(params)
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk=True)
    model = FloWaveNet(hp).load_params(params)
    lp, ld, zp = model.forward(dev(x), dev(c), return_z=True, lengths=lengths)
    z = z_planes_to_squeezed(zp, hp.n_block, hp.n_flow).cpu().numpy()
    lp, ld = lp.cpu().numpy(), ld.cpu().numpy()
    refs = {}
    for k, n in enumerate(lengths):
        refs[k] = onp.forward(p64, x[k:k + 1, :n].astype(np.float64), c[k:k + 1, :n // hp.hop_size].astype(np.float64), hp)
    # not vacuous: WITHOUT any masking (the fp64 oracle on the clip zero-padded to T) the shortest clip that is not full
    # differs from the clip alone by a multiple of the bound - reading across a clip's end is visible at these weights
    k = min((k for k, n in enumerate(lengths) if n < t), key=lambda k: lengths[k])
    n = lengths[k]
    xp, cp = np.zeros((1, t, 1)), np.zeros((1, t // hp.hop_size, hp.num_mels))
    xp[0, :n], cp[0, :n // hp.hop_size] = x[k, :n], c[k, :n // hp.hop_size]
    rows = n >> hp.n_block
    unmasked = float(np.abs(onp.forward(p64, xp, cp, hp)[2][:, :rows] - refs[k][2]).max())
    print("no masking at all (oracle, clip %d of %d samples zero-padded to %d): z off by %.3e = %.1f x ABS_Z" % (k, n, t, unmasked, unmasked / ABS_Z))
    assert unmasked >= 2.5 * ABS_Z, (cfg, unmasked)
    for k, n in enumerate(lengths):
        lp0, ld0, z0 = refs[k]
        rows = n >> hp.n_block
        err = float(np.abs(z[k:k + 1, :rows] - z0).max())
        print("clip %d (%d of %d samples): z max err %.3e, bound %.3e" % (k, n, t, err, ABS_Z))
        check_scalars(lp[k], ld[k], lp0, ld0)
        assert err <= ABS_Z, (cfg, k, n, err)
        assert not z[k, rows:].any()


def _loud_zero_conv(params):
    """The ZeroConv kernels times 5 (tests/test_ragged.py): the coupling then depends on the WaveNet's output strongly enough
    that what the front conv reads across a clip's end shows above the bound."""
    out = dict(params)
    for k in params:
        if "/ZeroConv1d/" in k and k.endswith("kernel"):
            out[k] = (params[k] * 5.0).astype(params[k].dtype)
    return out


@pytest.mark.parametrize("cfg,t,lengths", SMALL)
def test_each_clip_equals_the_oracle_at_loud_zero_convs(cfg, t, lengths):
    """The test above does not isolate the -shift fill of each flow's x_a plane: at the stock N(0, 0.02^2) ZeroConv kernels a
    pass WITHOUT that fill stays under ABS_Z (measured on an MI355X over these five cases: worst 0.92 x ABS_Z without the
    fill, 0.23 x with it).  With the kernels times 5 and z held to ``ABS_Z * max(1, |z0|max)`` the fill decides: without it
    every case misses (worst clip 1.40 - 2.76 x the bound), with it 0.19 - 0.48 x.  The scalars are held at the stock weights
    (above); at these the latent itself is tens of units wide and only z is compared."""
    hp = _hp(cfg)
    params = _loud_zero_conv(W.synthetic_params(hp, 99, actnorm="random"))
    p64 = onp.to_f64(params)
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk=True)
    model = FloWaveNet(hp).load_params(params)
    lp, ld, zp = model.forward(dev(x), dev(c), return_z=True, lengths=lengths)
    assert torch.isfinite(lp).all() and torch.isfinite(ld).all()
    z = z_planes_to_squeezed(zp, hp.n_block, hp.n_flow).cpu().numpy()
    for k, n in enumerate(lengths):
        z0 = onp.forward(p64, x[k:k + 1, :n].astype(np.float64), c[k:k + 1, :n // hp.hop_size].astype(np.float64), hp)[2]
        rows = n >> hp.n_block
        err, bound = float(np.abs(z[k:k + 1, :rows] - z0).max()), ABS_Z * max(1.0, float(np.abs(z0).max()))
        print("clip %d (%d of %d samples): z max err %.3e, bound %.3e" % (k, n, t, err, bound))
        assert err <= bound, (cfg, k, n, err, bound)
        assert not z[k, rows:].any()


@pytest.mark.parametrize("cfg,t,lengths", SMALL)
def test_round_trip(cfg, t, lengths):
    hp = _hp(cfg)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    x, c = _ragged_inputs(hp, len(lengths), t, lengths, junk=True)
    _, _, zp = model.forward(dev(x), dev(c), return_z=True, lengths=lengths)
    # planes [2][B][T/2] (even / odd samples) -> z [B][T][1], what reverse takes
    z = torch.stack([zp[0], zp[1]], dim=-1).reshape(len(lengths), t, 1)
    back = model.reverse(z, dev(c), lengths=lengths).cpu().numpy()
    for k, n in enumerate(lengths):
        bound = ABS_WAV * max(1.0, float(np.abs(x[k, :n]).max()))
        err = float(np.abs(back[k, :n] - x[k, :n]).max())
        print("clip %d (%d of %d samples): round trip max err %.3e, bound %.3e" % (k, n, t, err, bound))
        assert err <= bound, (cfg, k, n, err, bound)
        assert not back[k, n:].any()


def test_full_lengths_agree_with_the_plain_forward_and_leave_it_alone():
    """Every length = T: nothing is padding.  The ragged pass runs the saving tail (another template instantiation than the
    plain forward's), so the planes agree within the latent bound, not bit for bit; the batch means of the per-clip scalars
    are the plain forward's scalars."""
    hp = default_hparams()
    b, t = 3, 4096
    model = FloWaveNet(hp, chain_mode=1, persist_mode=1).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    inp = W.synthetic_inputs(hp, b, t, want=("x", "c"))
    x, c = dev(inp["x"]), dev(inp["c"])
    lp0, ld0, zp0 = model.forward(x, c, return_z=True)
    lp, ld, zp = model.forward(x, c, return_z=True, lengths=[t] * b)
    assert torch.isfinite(lp).all() and torch.isfinite(ld).all() and torch.isfinite(zp).all()
    check_scalars(lp.double().mean(), ld.double().mean(), float(lp0), float(ld0))
    err = float((zp - zp0).abs().max())
    print("planes against the plain forward: max diff %.3e, bound %.3e" % (err, ABS_Z))
    assert err <= ABS_Z
    again = model.forward(x, c, return_z=True)              # the plain pass is untouched by the ragged one before it
    assert torch.equal(again[0], lp0) and torch.equal(again[1], ld0) and torch.equal(again[2], zp0)


def test_full_size_clip_inside_a_ragged_batch_matches_the_committed_golden():
    """BASELINE configs[1]'s latency clip (the golden full_b8f6_B1_T16128) as clip 0 of a B = 4, T = 24 576 call."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    name = "full_b8f6_B1_T16128"
    over, b, t, actnorm, ddi = mg.CASES[name]
    hp = mg.hp_of(over)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = FloWaveNet(hp, init=True).load_params(W.synthetic_params(hp, 1234, actnorm=actnorm))
    inp = W.synthetic_inputs(hp, b, t)
    model.forward(dev(inp["x"]), dev(inp["c"]))              # the data-dependent ActNorm init from the golden's own clip
    big_t, lengths = 24576, [16128, 24576, 8192, 20480]
    x, c = _ragged_inputs(hp, 4, big_t, lengths, junk=True)
    x[0, :t], c[0, :t // hp.hop_size] = inp["x"][0], inp["c"][0]
    lp, ld, zp = model.forward(dev(x), dev(c), return_z=True, lengths=lengths)
    assert torch.isfinite(lp).all() and torch.isfinite(ld).all() and torch.isfinite(zp).all()
    check_scalars(lp[0], ld[0], float(g["log_p"]), float(g["logdet"]))
    assert not _planes_past_the_end(zp, lengths).any()


def _fill_case(lib, clips, rows, ch, spr, lens, offset):
    guard = 64
    n = clips * rows * ch
    rng = np.random.default_rng(rows * 131 + ch)
    host = rng.standard_normal(offset + n + guard).astype(np.float32)
    shift = rng.standard_normal(ch).astype(np.float32)
    shift[0] = 0.0                                                             # -(+0) + (+0) is +0 as well
    buf, sh = dev(host), dev(shift)
    assert buf.data_ptr() % 16 == 0
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    rc = lib.fwn_fill_neg_shift(buf.data_ptr() + 4 * offset, clips, rows, ch, sh.data_ptr(), ld.data_ptr(), spr, None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    want = host.copy()
    body = want[offset:offset + n].reshape(clips, rows, ch)
    for k, v in enumerate(lens):
        body[k, min(max(v, 0) // spr, rows):] = -shift
    got = buf.cpu().numpy()
    assert np.array_equal(got[:offset], host[:offset]) and np.array_equal(got[offset + n:], host[offset + n:])     # guards
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, ch, spr, lens, offset)
    # what it is for: ActNorm's (v + shift) of a filled row is exactly +0
    filled = torch.cat([buf[offset:offset + n].reshape(clips, rows, ch)[k, min(max(v, 0) // spr, rows):].reshape(-1, ch) for k, v in enumerate(lens)])
    assert np.array_equal((filled + sh).cpu().numpy().view(np.uint32), np.zeros(filled.shape, dtype=np.uint32))


def test_fill_neg_shift_kernel_alone():
    lib = _lib.load()
    for ch in (1, 2, 16, 128):
        spr = 2 * ch
        rows = 37
        # len 0, the whole plane, past it (clamped), one row, all but one row, negative - on every 4-byte phase of a 16-byte piece
        for offset in (0, 1, 2, 3):
            _fill_case(lib, 6, rows, ch, spr, [0, rows * spr, rows * spr + 1000, spr, (rows - 1) * spr, -5], offset)
    _fill_case(lib, 3, 8200, 1, 2, [2, 16400, 4102], 0)                      # more than one workgroup per clip
    _fill_case(lib, 3, 4100, 2, 4, [4, 16400, 8204], 1)
    _fill_case(lib, 2, 300, 128, 256, [256, 299 * 256], 0)
    _fill_case(lib, 1, 1, 1, 2, [0], 3)                                        # one dword


def _logdet_case(lib, clips, rows, ch, lens, offset=0):
    spr = 2 * ch
    rng = np.random.default_rng(rows * 17 + ch)
    z = rng.standard_normal((clips, rows, 2 * ch)).astype(np.float32)
    npt = max(1, ch // 32)
    ez = rng.uniform(0.5, 2.0, size=npt * 64).astype(np.float32)               # pair tiles: 32 log_s scales, then 32 t scales
    an = rng.standard_normal((2, 4, ch)).astype(np.float32)
    keep = [min(max(v, 0) // spr, rows) for v in lens]
    for k, r in enumerate(keep):
        z[k, r:] = np.nan                                                      # a padded row read into a sum would show
    tau = np.arange(ch)
    scale = ez[(tau // 32) * 64 + tau % 32].astype(np.float64)
    want = [-(z[k, :r, :ch].astype(np.float64) * scale).sum() for k, r in enumerate(keep)]
    mag = [np.abs(z[k, :r, :ch].astype(np.float64) * scale).sum() for k, r in enumerate(keep)]
    nslot = lib.fwn_ragged_logdet_slots(clips)
    zd = dev(np.concatenate([np.zeros(offset, dtype=np.float32), z.reshape(-1)]))
    acc = torch.full((clips, nslot), float("nan"), dtype=torch.float64, device="cuda")
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    ezd, and_ = dev(ez), dev(an)
    outs = []
    for _ in range(2):
        rc = lib.fwn_ragged_logdet_rows(zd.data_ptr() + 4 * offset, clips, rows, ch, ezd.data_ptr(), and_.data_ptr(), ld.data_ptr(), spr,
                                        acc.data_ptr(), None)
        assert rc == 0, lib.fwn_last_error()
        outs.append(acc.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])                                    # fixed-order sums: the same bits again
    got = outs[0]
    assert np.isfinite(got).all(), (rows, ch, lens)
    for k in range(clips):
        s = float(got[k, :nslot - 1].sum())
        assert abs(s - want[k]) <= 1e-6 * max(mag[k], 1e-30), (rows, ch, k, s, want[k])
        a = float((an[0, 3].astype(np.float64) + an[1, 3].astype(np.float64)).sum())
        assert abs(float(got[k, nslot - 1]) - a) <= 1e-12 * max(1.0, float(np.abs(an[:, 3]).sum()))


def test_ragged_logdet_kernel_alone():
    lib = _lib.load()
    for ch in (1, 2, 4, 16, 128):
        rows = 37
        spr = 2 * ch
        _logdet_case(lib, 6, rows, ch, [0, rows * spr, rows * spr + 1000, spr, (rows - 1) * spr, -5])
    _logdet_case(lib, 3, 70001, 1, [2, 140002, 70000])                       # many chunks per clip, odd rows (Ch = 1 pairs rows)
    _logdet_case(lib, 3, 33333, 2, [4, 133332, 40004])
    _logdet_case(lib, 2, 3000, 64, [128 * 2999, 128 * 1500])
    for ch in (1, 2, 4):                                                       # a base that is not 16-byte aligned
        _logdet_case(lib, 3, 41, ch, [2 * ch * 41, 2 * ch * 7, 0], offset=1)


def test_refusals():
    hp = small_hparams()
    params = W.synthetic_params(hp, 99, actnorm="random")
    model = FloWaveNet(hp).load_params(params)
    inp = W.synthetic_inputs(hp, 3, 64, want=("x", "c"))
    x, c = dev(inp["x"]), dev(inp["c"])
    for bad in BAD_LENGTHS:
        with pytest.raises(ValueError):
            model.forward(x, c, lengths=bad)
    lp, ld = model.forward(x, c, lengths=[64, 16, 48])
    assert lp.shape == ld.shape == (3,)
    with pytest.raises(ValueError, match="init"):
        FloWaveNet(hp, init=True).load_params(params).forward(x, c, lengths=[64, 16, 48])
    fp8 = FloWaveNet(hp, gate_fp8=True).load_params(params)
    with pytest.raises(ValueError, match="gate_fp8"):
        fp8.forward(x, c, lengths=[64, 16, 48])
    # the C entry point refuses such a descriptor, and null lengths, by itself
    lib = _lib.load()
    ld_ = torch.tensor([64, 16, 48], dtype=torch.int32).cuda()
    out = torch.empty(2, 3, device="cuda")
    x32, c32 = x.float().contiguous(), c.float().contiguous()
    for m, lens, word in ((fp8, ld_.data_ptr(), b"fp8"), (model, None, b"null lengths")):
        n = lib.fwn_ragged_forward_workspace_bytes(C.byref(m._packed.model_desc), 3, 64)
        assert n > lib.fwn_workspace_bytes(C.byref(m._packed.model_desc), 3, 64) > 0
        ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
        wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
        rc = lib.fwn_model_forward_ragged(C.byref(m._packed.model_desc), 3, 64, x32.data_ptr(), c32.data_ptr(), lens, wsp, n,
                                          out.data_ptr(), None, None)
        assert rc == -1 and word in lib.fwn_last_error(), lib.fwn_last_error()


def test_score_cli(tmp_path):
    """Every JSON line is the oracle's forward of that utterance alone, whichever batch it shared."""
    from tf_flowavenet_amd import score as SC
    from tf_flowavenet_amd import synthesize as S
    from tf_flowavenet_amd.hparams import hparams
    hp = hparams.replace(n_block=3, n_flow=2)
    params = W.synthetic_params(hp, 2, actnorm="random")
    for sub in ("ckpt", "audios", "mels"):
        (tmp_path / sub).mkdir()
    np.savez(tmp_path / "ckpt" / "flowavenet_model.npz", **params)
    rng = np.random.default_rng(0)
    clips = (("dataset-audio-00001.npy", "dataset-mel-00001.npy", 5), ("dataset-audio-00002.npy", "dataset-mel-00002.npy", 3),
             ("dataset-audio-00003.npy", "dataset-mel-00003.npy", 7))
    p64 = onp.to_f64(params)
    want, lines = {}, []
    for audio, mel, frames in clips:
        a = np.clip(0.3 * rng.standard_normal(frames * hp.hop_size), -0.999, 0.999).astype(np.float32)
        m = rng.random((frames, hp.num_mels), dtype=np.float32)
        np.save(tmp_path / "audios" / audio, a)
        np.save(tmp_path / "mels" / mel, m)
        lines.append("%s|%s|%d|0|text" % (audio, mel, len(a)))
        want[audio] = onp.forward(p64, a.astype(np.float64)[None, :, None], m.astype(np.float64)[None], hp)[:2]
    (tmp_path / "train.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    assert len(S.plan_batches([f for _, _, f in clips], 8, 0.6, hp)) < len(clips)          # clips do share a call at --batch 8
    for batch in (1, 8):
        out = tmp_path / ("scores%d.jsonl" % batch)
        args = type("A", (), dict(saved_dir=str(tmp_path / "ckpt"), base_dir=str(tmp_path), out=str(out), batch=batch, max_pad_frac=0.6))()
        recs = SC.score(args, hp)
        read = [json.loads(line) for line in out.read_text(encoding="utf-8").splitlines()]
        assert read == recs and [r["name"] for r in read] == [a for a, _, _ in clips]      # train.txt's order
        for r, (audio, _, frames) in zip(read, clips):
            assert r["samples"] == frames * hp.hop_size
            check_scalars(r["log_p"], r["logdet"], *want[audio])
            assert r["nll"] == -(r["log_p"] + r["logdet"])
