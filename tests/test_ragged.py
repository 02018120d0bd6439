"""Ragged batches (-m gpu): ``FloWaveNet.reverse(z, c, lengths=)`` gives every clip of a batch what that clip gives alone,
whatever the batch holds past the clip's end.

Tolerances: a clip against the fp64 oracle's reverse of that clip alone is held to the suite's waveform bound
(tests/test_gpu_parity.py: ``ABS_WAV * max(1, |x0|max)``, bf16 hidden activations with fp32 accumulation); statements about
the padding (inert, zero output) and about full lengths are exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams, hparams8000
from tf_flowavenet_amd.model import FloWaveNet

from conftest import small_hparams

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABS_WAV = 1e-2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _loud_zero_conv(params):
    """The ZeroConv kernels times 5: the coupling then depends on the WaveNet's output strongly enough that a row read
    across a clip's end shows far above the bound (at the stock N(0, 0.02^2) it is 6 - 9 times the bound already)."""
    out = dict(params)
    for k in params:
        if "/ZeroConv1d/" in k and k.endswith("kernel"):
            out[k] = (params[k] * 5.0).astype(params[k].dtype)
    return out


def _ragged_inputs(hp, b, t, lengths, junk):
    """z, c of W.synthetic_inputs with the part past each clip's length replaced: zeros, or junk (z: 3 N(0,1), mel: 1.0)."""
    inp = W.synthetic_inputs(hp, b, t, want=("c", "z"))
    z, c = inp["z"].copy(), inp["c"].copy()
    rng = np.random.default_rng(5)
    for k, n in enumerate(lengths):
        z[k, n:] = 3.0 * rng.standard_normal(z[k, n:].shape) if junk else 0.0
        c[k, n // hp.hop_size:] = 1.0 if junk else 0.0
    return z.astype(np.float32), c.astype(np.float32)


SMALL = [
    (dict(), 256, [256, 16, 160, 96]),
    (dict(n_block=4, n_flow=2), 256, [160, 256, 16, 208]),
    (dict(n_block=2, n_flow=4, n_layer=4), 192, [192, 16, 64, 112]),                   # dilation 27 reaches past the short clips
    (dict(n_block=5, n_flow=2, num_mels=16, hop_size=32, upsample_scales=[4, 8]), 128, [32, 128, 64, 96]),   # one row at the last block
    ("8k", 480, [480, 96, 192, 384]),                                                    # hparams8000's geometry: hop 96 = 8 x 12, n_block 5
]


def _hp(cfg):
    return hparams8000().replace(n_flow=2, num_mels=16) if cfg == "8k" else small_hparams(**cfg)


@pytest.mark.parametrize("cfg,t,lengths", SMALL + [("full", 4096, [4096, 256, 2048, 3072])])
def test_padding_is_inert_bit_for_bit(cfg, t, lengths):
    hp = default_hparams() if cfg == "full" else _hp(cfg)
    model = FloWaveNet(hp).load_params(_loud_zero_conv(W.synthetic_params(hp, 99, actnorm="random")))
    outs = []
    for junk in (False, True):
        z, c = _ragged_inputs(hp, len(lengths), t, lengths, junk)
        zd, cd = dev(z), dev(c)
        keep = (zd.clone(), cd.clone())
        outs.append(model.reverse(zd, cd, lengths=lengths))
        assert torch.equal(zd, keep[0]) and torch.equal(cd, keep[1])          # the caller's z and c are never written
    assert outs[0].shape == (len(lengths), t, 1)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    for k, n in enumerate(lengths):
        assert float(outs[1][k, :n].abs().max()) > 0.0
        assert not outs[1][k, n:].any(), (k, n)                             # exactly 0 past the clip
    # lengths as a NumPy array, a CPU tensor and a device tensor are the same call
    z, c = _ragged_inputs(hp, len(lengths), t, lengths, True)
    for form in (np.asarray(lengths), torch.tensor(lengths), torch.tensor(lengths, dtype=torch.int32).cuda()):
        assert torch.equal(model.reverse(dev(z), dev(c), lengths=form), outs[1])


@pytest.mark.parametrize("cfg,t,lengths", SMALL)
def test_each_clip_equals_the_oracle_reverse_of_that_clip_alone(cfg, t, lengths):
    hp = _hp(cfg)
    unit = int(np.lcm(hp.hop_size, 1 << hp.n_block))
    assert t in lengths and unit in lengths                                   # T itself and the shortest legal clip
    params = _loud_zero_conv(W.synthetic_params(hp, 99, actnorm="random"))
    p64 = onp.to_f64(params)
    z, c = _ragged_inputs(hp, len(lengths), t, lengths, junk=True)
    model = FloWaveNet(hp).load_params(params)
    out = model.reverse(dev(z), dev(c), lengths=lengths).cpu().numpy()
    for k, n in enumerate(lengths):
        x0 = onp.reverse(p64, z[k:k + 1, :n].astype(np.float64), c[k:k + 1, :n // hp.hop_size].astype(np.float64), hp)
        err = float(np.abs(out[k:k + 1, :n] - x0).max())
        bound = ABS_WAV * max(1.0, float(np.abs(x0).max()))
        print("clip %d (%d of %d samples): max err %.3e, bound %.3e" % (k, n, t, err, bound))
        assert err <= bound, (cfg, k, n, err, bound)
        assert not out[k, n:].any()


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
    half_ulp = 2.0 ** -11 if g["x_rev"].dtype == np.float16 else 0.0
    model = FloWaveNet(hp, init=True).load_params(W.synthetic_params(hp, 1234, actnorm=actnorm))
    inp = W.synthetic_inputs(hp, b, t)
    model.forward(dev(inp["x"]), dev(inp["c"]))              # the data-dependent ActNorm init from the golden's own clip
    big_t, lengths = 24576, [16128, 24576, 8192, 20480]
    z, c = _ragged_inputs(hp, 4, big_t, lengths, junk=True)
    z[0, :t], c[0, :t // hp.hop_size] = inp["z"][0], inp["c"][0]
    out = model.reverse(dev(z), dev(c), lengths=lengths).cpu().numpy()
    x0 = g["x_rev"].astype(np.float32)
    wav = out[0:1, :t]
    assert wav.shape == x0.shape
    scale = max(1.0, float(np.abs(x0).max()))
    err = np.abs(wav - x0)
    print("clip 0 against the golden: max err %.3e (bound %.3e), mean %.3e (bound %.3e)" % (err.max(), ABS_WAV * scale, err.mean(), 1e-3 * scale))
    assert (err <= ABS_WAV * scale + half_ulp * np.abs(x0)).all(), err.max()
    assert err.mean() < 1e-3 * scale
    for k, n in enumerate(lengths):
        assert not out[k, n:].any()
    assert np.isfinite(out).all()


@pytest.mark.parametrize("b,t", [(8, 16128), (3, 4096)])
def test_full_lengths_change_nothing(b, t):
    """With every length = T the masks zero nothing, and the stage sequence is that of a model without chaining and without
    one-launch flows: the same bits."""
    hp = default_hparams()
    model = FloWaveNet(hp, chain_mode=1, persist_mode=1).load_params(W.synthetic_params(hp, 1234, actnorm="random"))
    inp = W.synthetic_inputs(hp, b, t, want=("c", "z"))
    z, c = dev(inp["z"]), dev(inp["c"])
    plain = model.reverse(z, c)
    ragged = model.reverse(z, c, lengths=[t] * b)
    assert torch.isfinite(plain).all()
    assert torch.equal(plain, ragged)
    assert torch.equal(model.reverse(z, c), plain)            # and the plain pass is untouched by the ragged one before it


def _mask_case(lib, clips, rows, row_bytes, spr, lens, offset):
    guard = 256
    n = clips * rows * row_bytes
    rng = np.random.default_rng(rows * 131 + row_bytes)
    host = rng.integers(1, 256, size=offset + n + guard, dtype=np.uint8)        # no zero byte anywhere before the call
    buf = torch.from_numpy(host.copy()).cuda()
    assert buf.data_ptr() % 16 == 0
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    rc = lib.fwn_mask_rows(buf.data_ptr() + offset, clips, rows, row_bytes, ld.data_ptr(), spr, None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    want = host.copy()
    body = want[offset:offset + n].reshape(clips, rows, row_bytes)
    for k, v in enumerate(lens):
        body[k, min(max(v, 0) // spr, rows):] = 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:offset], host[:offset]) and np.array_equal(got[offset + n:], host[offset + n:])     # guards
    assert np.array_equal(got, want), (rows, row_bytes, spr, lens, offset)


def test_mask_rows_kernel_alone():
    lib = _lib.load()
    # bf16 [B][rows][256]: h of a block with 2 Ch = 8 samples per row; len 0, the whole buffer, past it (clamped), negative
    _mask_case(lib, 6, 37, 512, 8, [0, 37 * 8, 37 * 8 + 1000, 8, 36 * 8, -5], 0)
    _mask_case(lib, 3, 4100, 512, 2, [2, 8200, 4102], 0)                      # more than one workgroup per clip
    # fp32 rows of an odd number of floats, the buffer itself on every 4-byte phase of a 16-byte piece: dword heads and tails
    for floats in (1, 3, 5, 7, 13, 81):
        for offset in (0, 4, 8, 12):
            rows = 29
            _mask_case(lib, 5, rows, 4 * floats, 3, [0, rows * 3, rows * 3 + 7, 3 * 11 + 2, 3 * 28], offset)
    _mask_case(lib, 16, 8064, 4, 2, [16128 - 256 * k for k in range(16)], 4)  # the flow-state planes of a B = 8 call
    _mask_case(lib, 1, 1, 4, 1, [0], 12)                                        # one dword


def test_bad_lengths_raise_value_error():
    hp = small_hparams()
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    inp = W.synthetic_inputs(hp, 3, 64, want=("c", "z"))
    z, c = dev(inp["z"]), dev(inp["c"])
    for bad in ([64, 64], [64, 64, 64, 64], [64, 24, 64], [64, 80, 64], [64, 0, 64], [64, 8, 64], [64, -16, 64], [64, 32.5, 64], 64):
        with pytest.raises(ValueError):
            model.reverse(z, c, lengths=bad)
    assert model.reverse(z, c, lengths=[64, 16, 48]).shape == (3, 64, 1)
    fp8 = FloWaveNet(hp, gate_fp8=True).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    with pytest.raises(ValueError, match="gate_fp8"):
        fp8.reverse(z, c, lengths=[64, 16, 48])
    # the C entry point refuses such a descriptor by itself
    lib = _lib.load()
    n = lib.fwn_ragged_workspace_bytes(C.byref(fp8._packed.model_desc), 3, 64)
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    ld = torch.tensor([64, 16, 48], dtype=torch.int32).cuda()
    x = torch.empty(3, 64, 1, device="cuda")
    z32, c32 = z.float().contiguous(), c.float().contiguous()
    wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
    rc = lib.fwn_model_reverse_ragged(C.byref(fp8._packed.model_desc), 3, 64, z32.data_ptr(), c32.data_ptr(), ld.data_ptr(), wsp, n,
                                      x.data_ptr(), None)
    assert rc == -1 and b"fp8" in lib.fwn_last_error()


def test_synthesize_cli_ragged(tmp_path):
    """``--ragged``: every wav is the oracle's reverse of that clip alone with the clip's own seeded z, whichever batch it
    shared (the PCM comparison of test_synthesize_cli_file_contract)."""
    import wave
    from tf_flowavenet_amd import synthesize as S
    from tf_flowavenet_amd.hparams import hparams
    hp = hparams.replace(n_block=3, n_flow=2)
    params = W.synthetic_params(hp, 2, actnorm="random")
    (tmp_path / "ckpt").mkdir()
    (tmp_path / "mels").mkdir()
    np.savez(tmp_path / "ckpt" / "flowavenet_model.npz", **params)
    rng = np.random.default_rng(0)
    clips = (("a", 5), ("b", 3), ("c", 7), ("d", 4))
    for name, frames in clips:
        np.save(tmp_path / "mels" / (name + ".npy"), rng.random((frames, 80), dtype=np.float32))
    p64 = onp.to_f64(params)
    want = {}
    for k, (name, frames) in enumerate(clips):                      # k: the clip's index in sorted file-name order
        gen = torch.Generator(device="cpu").manual_seed(75 + k)
        z = (torch.randn(frames * 256, 1, generator=gen) * hp.temp).numpy().astype(np.float64)[None]
        c = np.load(tmp_path / "mels" / (name + ".npy")).astype(np.float64)[None]
        want[name] = onp.reverse(p64, z, c, hp)[0, :, 0]
    assert len(S.plan_batches([f for _, f in clips], 8, 0.25, hp)) < len(clips)       # clips do share calls at --batch 8
    for batch in (1, 8):
        out = tmp_path / ("out%d" % batch)
        args = type("A", (), dict(saved_dir=str(tmp_path / "ckpt"), mels_dir=str(tmp_path / "mels"), output_dir=str(out), seed=75,
                                  batch=batch, ragged=True, max_pad_frac=0.25))()
        assert S.synthesize(args, hp) == ["a.npy", "b.npy", "c.npy", "d.npy"]
        for name, frames in clips:
            with wave.open(str(out / (name + ".wav"))) as w:
                assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 22050)
                assert w.getnframes() == frames * 256
                pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64)
            ref = np.clip(want[name], -1.0, 1.0) * 32767.0
            tol = 1.0 + ABS_WAV * max(1.0, float(np.abs(want[name]).max())) * 32767.0      # one LSB of rounding + the waveform tolerance
            assert np.abs(pcm - ref).max() <= tol, (batch, name, np.abs(pcm - ref).max(), tol)
