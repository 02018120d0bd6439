"""GPU tests of the spectral distances (csrc/specdist.hip) against tests/specdist_ref.py: every refusal, the mel
term against the device's own ``fwn_mel_front`` mels, identity and gain, the three measures inside the restatement's bound at
every shape and edge length, the locality rule (a ragged batch = every pair alone, bit for bit), offsets past 2^31, and the
surfaces: ``metrics.SpectralDistance``, the ``evaluate`` CLI in both modes, ``train.py --eval_metrics``."""
import json
import os
import wave
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mel_front_ref as MR
import specdist_ref as R
from conftest import small_hparams
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import evaluate as E
from tf_flowavenet_amd import preprocessing as P
from tf_flowavenet_amd.metrics import SpectralDistance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 777.25
GUARD = 16


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


_TABLES = {}


def _tables(hp):
    key = (hp.n_fft, hp.hop_size, hp.num_mels)
    if key not in _TABLES:
        fb = P.mel_filterbank(hp)
        _TABLES[key] = (fb, torch.from_numpy(fb).to(DEV), torch.from_numpy(P.mel_bands(fb)).to(DEV))
    return _TABLES[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(lib, pairs, n_fft, hop, hp=None, bands=True, len_host=None, len_dev=True, pad=(3, 6), floor=R.FLOOR):
    """fwn_spectral_distance over ``pairs`` in one ragged call: NaN behind every clip's end in both inputs, odd strides (rows at
    every alignment), junk in ``out`` and in the workspace, sentinel doubles around ``out`` (checked here).  -> [B, 4] fp64."""
    B = len(pairs)
    lens = [len(a) for a, _ in pairs]
    L = len_host or max(max(lens), 1)
    xs, ys = L + pad[0], L + pad[1]
    hx, hy = np.full(B * xs, np.nan, dtype=np.float32), np.full(B * ys, np.nan, dtype=np.float32)
    for b, (a, c) in enumerate(pairs):
        assert len(a) == len(c)
        hx[b * xs:b * xs + len(a)] = a
        hy[b * ys:b * ys + len(c)] = c
    x, y = torch.from_numpy(hx).to(DEV), torch.from_numpy(hy).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int64, device=DEV) if len_dev else None
    assert len_dev or all(n == L for n in lens)
    out = torch.full((GUARD + B * 4 + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    out[GUARD:GUARD + B * 4] = float("nan") if B % 2 else -1e300                   # junk
    wsb = int(lib.fwn_spectral_distance_workspace_bytes(B, L, n_fft, hop))
    assert wsb == B * (-(-(1 + L // hop) // R.FRAMES)) * 32
    ws = torch.full((wsb // 8 + 1,), float("nan") if len(pairs[0][0]) % 2 else 1e300, dtype=torch.float64, device=DEV)
    fb = bd = None
    if hp is not None:
        _, fb, bd = _tables(hp)
    rc = lib.fwn_spectral_distance(x.data_ptr(), xs, y.data_ptr(), ys, B, None if ld is None else ld.data_ptr(), L,
                                   None if fb is None else fb.data_ptr(), bd.data_ptr() if (fb is not None and bands) else None,
                                   n_fft, hop, hp.num_mels if hp is not None else 0, float(hp.ref_level_db) if hp is not None else 0.0,
                                   float(hp.min_level_db) if hp is not None else 0.0, floor, out.data_ptr() + 8 * GUARD, ws.data_ptr(),
                                   wsb, None)
    _lib.check(rc, "fwn_spectral_distance")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:GUARD] == SENTINEL) and np.all(o[GUARD + B * 4:] == SENTINEL)
    return o[GUARD:GUARD + B * 4].reshape(B, 4)


# ---- refusals ----
def test_every_refusal_comes_before_any_launch(lib):
    for kw, word in R.REFUSALS:
        assert R.refusal_call(lib, **kw) == -1, kw
        msg = lib.fwn_last_error()
        assert b"fwn_spectral_distance" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()                                   # nothing was launched at those addresses: no fault to report
    x, y = R.pair(1, 700)
    got = _run(lib, [(x, y)], 64, 16)                          # without fb, n_mels = 0 and min_level_db = 0 are accepted
    assert np.isnan(got[0, 0]) and np.isfinite(got[0, 1:]).all() and got[0, 3] == 1 + 700 // 16


# ---- the mel term is fwn_mel_front's ----
@pytest.mark.parametrize("n_fft,hop,n_mels,n", [(1024, 256, 80, 7001), (64, 16, 8, 1000), (256, 100, 20, 1501), (2048, 512, 16, 9000)])
def test_mel_term_is_the_front_ends_own(lib, n_fft, hop, n_mels, n):
    """The mels of x and of y from ``fwn_mel_front(peak NULL)`` itself, |difference| in float32 as the kernel forms it, summed in
    fp64 on the host: only the order of that sum may differ from the kernel's."""
    hp = MR.hp_of(n_fft, hop, n_mels)
    x, y = R.pair(n, n)
    _, fb, bd = _tables(hp)
    F = 1 + n // hop
    mels = []
    for c in (x, y):
        cd = torch.from_numpy(c).to(DEV)
        mel = torch.empty(F * n_mels, dtype=torch.float32, device=DEV)
        _lib.check(lib.fwn_mel_front(cd.data_ptr(), 1, n, None, n, None, 1.0, fb.data_ptr(), bd.data_ptr(), n_fft, hop, n_mels,
                                     float(hp.ref_level_db), float(hp.min_level_db), mel.data_ptr(), F * n_mels, None, 0, None),
                   "fwn_mel_front")
        mels.append(mel.cpu().numpy())
    d32 = np.abs(mels[0] - mels[1])
    assert d32.dtype == np.float32 and d32.max() > 0
    want = float(d32.astype(np.float64).sum() / (F * n_mels))
    got = _run(lib, [(x, y)], n_fft, hop, hp)[0]
    print("n_fft %d: mel_l1 %.17g, from fwn_mel_front's mels %.17g" % (n_fft, got[0], want))
    assert got[3] == F and abs(got[0] - want) <= F * n_mels * 2.0 ** -53 * want


# ---- identity and gain ----
@pytest.mark.parametrize("n_fft,hop,n_mels", R.SHAPES)
def test_identity_is_exactly_zero(lib, n_fft, hop, n_mels):
    hp = MR.hp_of(n_fft, hop, n_mels)
    clips = [MR.signal(n, n) for n in (n_fft // 2 + 1, R.FRAMES * hop + 1, 3 * R.FRAMES * hop)]
    got = _run(lib, [(c, c) for c in clips], n_fft, hop, hp)
    for row, c in zip(got, clips):
        assert not _bits(row[:3]).any() and row[3] == 1 + len(c) // hop, row      # +0, all three


@pytest.mark.parametrize("n_fft,hop,n_mels,n", [(1024, 256, 80, 1500), (512, 128, 40, 1300), (2048, 512, 32, 5000)])
def test_half_gain_sits_at_its_known_answers(lib, n_fft, hop, n_mels, n):
    """y = 0.5 x on noise whose every bin and mel is clear of the floor and the clip: sc = 0.5, lsd_db = 20 log10 2 and
    mel_l1 = 2 * 20 log10 2 / -min_level_db (the front-end's mel is 20 log10 of a POWER), each within the bound."""
    hp = MR.hp_of(n_fft, hop, n_mels)
    fb = _tables(hp)[0]

    def noise(s):
        return (0.1 * np.random.default_rng(s).standard_normal(n)).astype(np.float32)

    def plain(s):
        half = np.float32(0.5) * noise(s)
        return R.power64(half, n_fft, hop).min() > R.FLOOR and R.mel64(half, hp, fb).min() > 0.0
    x = noise(next(s for s in range(100) if plain(s)))
    y = np.float32(0.5) * x
    assert R.mel64(x, hp, fb).max() < 1.0
    got = _run(lib, [(x, y)], n_fft, hop, hp)[0]
    bd = R.bound(x, y, n_fft, hop, hp, fb)
    want = (2 * 20 * np.log10(2.0) / -hp.min_level_db, 20 * np.log10(2.0), 0.5)
    sh = R.shares(got, want, bd)
    print("n_fft %d: half gain at %.4f / %.4f / %.4f of the bound" % ((n_fft,) + tuple(sh)))
    assert max(sh) <= 1.0, (got, want, bd)
    zero = _run(lib, [(x, np.zeros_like(x)), (np.zeros_like(x), x), (np.zeros_like(x), np.zeros_like(x))], n_fft, hop, hp)
    assert abs(zero[0, 2] - 1.0) <= bd[2] and zero[1, 2] == float("inf") and np.isnan(zero[2, 2])     # the IEEE quotient is kept
    assert zero[2, 0] == 0.0 and zero[2, 1] == 0.0


# ---- against the restatement ----
SHARES = {}


@pytest.mark.parametrize("n_fft,hop,n_mels", R.SHAPES)
def test_against_the_restatement(lib, n_fft, hop, n_mels):
    hp = MR.hp_of(n_fft, hop, n_mels)
    fb = _tables(hp)[0]
    lens = R.lengths_of(n_fft, hop)
    pairs = [R.pair(n, n) for n in lens]
    got = _run(lib, pairs, n_fft, hop, hp)
    worst, worst32 = [0.0] * 3, [0.0] * 3
    for row, (x, y) in zip(got, pairs):
        ref, bd = R.dist(x, y, n_fft, hop, hp, fb), R.bound(x, y, n_fft, hop, hp, fb)
        sh, sh32 = R.shares(row, ref, bd), R.shares(R.dist32(x, y, n_fft, hop, hp, fb), ref, bd)
        print("n_fft %d hop %d N %d: kernel at %.4f / %.4f / %.4f of the bound, float32 NumPy at %.4f / %.4f / %.4f"
              % ((n_fft, hop, len(x)) + tuple(sh) + tuple(sh32)))
        worst, worst32 = [max(a, b) for a, b in zip(worst, sh)], [max(a, b) for a, b in zip(worst32, sh32)]
        assert row[3] == ref[3] == 1 + len(x) // hop
        assert max(sh) <= 1.0, (len(x), row, ref, bd)
    print("n_fft %d hop %d n_mels %d WORST: kernel %.4f / %.4f / %.4f, float32 NumPy %.4f / %.4f / %.4f (mel_l1 / lsd_db / sc)"
          % ((n_fft, hop, n_mels) + tuple(worst) + tuple(worst32)))
    other = _run(lib, pairs[:3], n_fft, hop, None, floor=1e-2)                     # another floor, no fb: lsd alone moves
    for row, full, (x, y) in zip(other, got, pairs):
        ref, bd = R.dist(x, y, n_fft, hop, floor=1e-2), R.bound(x, y, n_fft, hop, floor=1e-2)
        assert np.isnan(row[0]) and _bits(row[2]) == _bits(full[2]) and abs(row[1] - ref[1]) <= bd[1]


# ---- ragged rows and robustness ----
@pytest.mark.parametrize("n_fft,hop,n_mels", [(1024, 256, 80), (256, 100, 20), (64, 16, 8), (2048, 512, 16)])
def test_a_ragged_batch_is_every_pair_alone(lib, n_fft, hop, n_mels):
    hp = MR.hp_of(n_fft, hop, n_mels)
    lens = [n_fft // 2 + 1, 5 * hop + 7, R.FRAMES * hop, 2 * R.FRAMES * hop + 3, 3 * R.FRAMES * hop + hop // 2]
    pairs = [R.pair(10 + n, n) for n in lens]
    alone = np.stack([_run(lib, [p], n_fft, hop, hp, len_dev=False, pad=(0, 0))[0] for p in pairs])
    assert np.isfinite(alone).all() and (alone[:, :3] > 0).all()
    batch = _run(lib, pairs, n_fft, hop, hp)                   # NaN past every end, junk in out and the workspace: _run
    assert np.array_equal(_bits(batch), _bits(alone))
    assert np.array_equal(_bits(_run(lib, pairs, n_fft, hop, hp, bands=False)), _bits(alone))
    assert np.array_equal(_bits(_run(lib, pairs[::-1], n_fft, hop, hp, len_host=max(lens) + 5 * hop + 1, pad=(8, 1))), _bits(alone[::-1]))
    # a pair too short to reflect among live ones: NaN and 0 frames, and its neighbours are unchanged
    short = (pairs[1][0][:n_fft // 2], pairs[1][1][:n_fft // 2])
    empty = (pairs[1][0][:0], pairs[1][1][:0])
    mixed = _run(lib, [pairs[0], short, pairs[3], empty, pairs[4]], n_fft, hop, hp)
    assert np.array_equal(_bits(mixed[[0, 2, 4]]), _bits(alone[[0, 3, 4]]))
    for row in (mixed[1], mixed[3]):
        assert np.isnan(row[:3]).all() and row[3] == 0.0
    # x and y may be one buffer
    c = torch.from_numpy(pairs[3][0]).to(DEV)
    out = torch.empty(4, dtype=torch.float64, device=DEV)
    n = len(pairs[3][0])
    ws = torch.empty(int(lib.fwn_spectral_distance_workspace_bytes(1, n, n_fft, hop)) // 8, dtype=torch.float64, device=DEV)
    _lib.check(lib.fwn_spectral_distance(c.data_ptr(), n, c.data_ptr(), n, 1, None, n, None, None, n_fft, hop, 0, 0.0, 0.0, 1e-4,
                                         out.data_ptr(), ws.data_ptr(), ws.numel() * 8, None), "fwn_spectral_distance")
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and o[1] == 0.0 and o[2] == 0.0 and o[3] == 1 + n // hop


# ---- 64-bit offsets ----
def test_rows_past_2_to_the_31(lib):
    """One buffer of 2^31 + 8 + 5001 floats; x = buf, y = buf + 1: the test clip is the target shifted by one sample; two rows
    2^31 + 8 apart, so row 1 lies past element 2^31."""
    n_fft, hop, n_mels, n = 1024, 256, 80, 5000
    hp = MR.hp_of(n_fft, hop, n_mels)
    fb, fbd, bd = _tables(hp)
    stride = (1 << 31) + 8
    free, _ = torch.cuda.mem_get_info()
    if free < (stride + n + 1) * 4 + (1 << 30):
        pytest.fail("needs %.1f GB of device memory" % ((stride + n + 1) * 4 / 1e9))
    buf = torch.empty(stride + n + 1, dtype=torch.float32, device=DEV)
    clips = [MR.signal(41, n + 1), MR.signal(42, n + 1)]
    for b in (0, 1):
        buf[b * stride:b * stride + n + 1] = torch.from_numpy(clips[b]).to(DEV)
    out = torch.empty(8, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.fwn_spectral_distance_workspace_bytes(2, n, n_fft, hop)) // 8, dtype=torch.float64, device=DEV)
    _lib.check(lib.fwn_spectral_distance(buf.data_ptr(), stride, buf.data_ptr() + 4, stride, 2, None, n, fbd.data_ptr(), bd.data_ptr(),
                                         n_fft, hop, n_mels, float(hp.ref_level_db), float(hp.min_level_db), 1e-4, out.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 8, None), "fwn_spectral_distance")
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(2, 4)
    del buf
    torch.cuda.empty_cache()
    for b in (0, 1):
        x, y = clips[b][:n], clips[b][1:]
        ref, bnd = R.dist(x, y, n_fft, hop, hp, fb), R.bound(x, y, n_fft, hop, hp, fb)
        sh = R.shares(got[b], ref, bnd)
        print("row %d: %.4f / %.4f / %.4f of the bound" % ((b,) + tuple(sh)))
        assert max(sh) <= 1.0 and got[b, 3] == 1 + n // hop and ref[2] > 0.01
        assert np.array_equal(_bits(got[b]), _bits(_run(lib, [(x, y)], n_fft, hop, hp)[0]))      # the row it is in a small buffer


# ---- the Python surface ----
def test_spectral_distance_object(lib):
    hp = MR.hp_of(256, 64, 20)
    fb = _tables(hp)[0]
    res = [(128, 32), (256, 64), (512, 128)]
    sd = SpectralDistance(hp, res, device=DEV)
    lens = [3000, 1200, 700]
    pairs = [R.pair(50 + n, n) for n in lens]
    x, _ = P.ragged_rows([p[0] for p in pairs], DEV)
    y, _ = P.ragged_rows([p[1] for p in pairs], DEV)
    d = sd.dist(x, y, lengths=torch.tensor(lens, device=DEV))
    assert set(d) == {"mel_l1", "lsd_db", "sc", "frames"} | {"%s@%d/%d" % (m, n, h) for m in ("lsd_db", "sc") for n, h in res}
    assert all(v.dtype == torch.float64 and v.shape == (3,) and v.is_cuda for v in d.values())
    d = {k: v.cpu().numpy() for k, v in d.items()}
    for b, (a, c) in enumerate(pairs):
        per = [R.dist(a, c, n, h, hp if (n, h) == (256, 64) else None, fb if (n, h) == (256, 64) else None) for n, h in res]
        bds = [R.bound(a, c, n, h, hp if (n, h) == (256, 64) else None, fb if (n, h) == (256, 64) else None) for n, h in res]
        assert d["frames"][b] == 1 + lens[b] // 64 and abs(d["mel_l1"][b] - per[1][0]) <= bds[1][0]
        for (n, h), r, bd in zip(res, per, bds):
            assert abs(d["lsd_db@%d/%d" % (n, h)][b] - r[1]) <= bd[1] and abs(d["sc@%d/%d" % (n, h)][b] - r[2]) <= bd[2]
        assert abs(d["lsd_db"][b] - np.mean([r[1] for r in per])) <= np.mean([bd[1] for bd in bds])
        assert abs(d["sc"][b] - np.mean([r[2] for r in per])) <= np.mean([bd[2] for bd in bds])
    one = sd.dist(torch.from_numpy(pairs[1][0]).to(DEV), torch.from_numpy(pairs[1][1]).to(DEV))       # [T]: alone, the same bits
    assert all(_bits(one[k].cpu().numpy()[0]) == _bits(d[k][1]) for k in d)
    assert len(sd._ws) == 6 and SpectralDistance(hp, device=DEV).resolutions == [(256, 64)]
    with pytest.raises(TypeError):
        sd.dist(x.double(), y.double())
    with pytest.raises(ValueError):
        sd.dist(x, y[:, :-1])
    with pytest.raises(ValueError):
        SpectralDistance(hp, [(100, 10)], device=DEV)


# ---- end to end ----
def _write_wav(path, x, rate):
    pcm = (np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def _corpus(root, hp, frame_counts, seed=0):
    rng = np.random.default_rng(seed)
    for sub in ("audios", "mels"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    lines = []
    for k, f in enumerate(frame_counts):
        audio = (0.3 * rng.standard_normal(f * hp.hop_size)).astype(np.float32)
        np.save(os.path.join(root, "audios", "u%d-audio.npy" % k), audio)
        np.save(os.path.join(root, "mels", "u%d-mel.npy" % k), rng.random((f, hp.num_mels)).astype(np.float32))
        lines.append("u%d-audio.npy|u%d-mel.npy|%d|0|text" % (k, k, len(audio)))
    with open(os.path.join(root, "train.txt"), "wt", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


def test_evaluate_copy_synthesis(tmp_path):
    """Every record against the restatement applied to what ``synthesize(..., return_wav=True)`` returns for that clip alone at
    the same seed and clip id - after ``Denoiser`` with ``--denoise``, through ``synthesize_windowed`` for the long utterance
    with ``--window`` - inside ``bound()``."""
    from tf_flowavenet_amd import score as SC
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.denoise import Denoiser
    from tf_flowavenet_amd.model import FloWaveNet
    hp = small_hparams(n_fft=64)
    fb = P.mel_filterbank(hp)
    frames = [40, 57, 48, 130]
    _corpus(str(tmp_path), hp, frames)
    model = FloWaveNet(hp, device=DEV).load_params(W.synthetic_params(hp, 4321, actnorm="random"))
    hop, seed = hp.hop_size, 77
    res = [(64, 16), (128, 32)]
    for tag, extra in (("plain", []), ("denoise", ["--denoise", "0.5"]), ("window", ["--window", "512"])):
        out_path = str(tmp_path / (tag + ".jsonl"))
        args = E.parse_args(["--saved_dir", "unused/", "--base_dir", str(tmp_path), "--out", out_path, "--seed", str(seed), "--batch", "3",
                             "--resolutions", "64/16,128/32"] + extra)
        out, summary = E.evaluate_synthesis(args, hp, model=model, device=DEV)
        assert [r["name"] for r in out] == ["u%d-audio.npy" % k for k in range(4)]
        assert [json.loads(s) for s in open(out_path)] == out + [summary] and summary["utterances"] == 4
        dn = Denoiser(model, strength=0.5) if tag == "denoise" else None
        for k, r in enumerate(out):
            f = SC.cropped_frames(frames[k], hp)
            n = f * hop
            c = torch.from_numpy(np.load(tmp_path / "mels" / ("u%d-mel.npy" % k))[None, :f]).to(DEV)
            if tag == "window" and n > 512:
                wav = model.synthesize_windowed(c, seed, clip_ids=[k], window=512, batch=3, return_wav=True)[1]
            else:
                wav = model.synthesize(c, seed, clip_ids=[k], lengths=[n], return_wav=True)[1]
            y = wav[:, :, 0].contiguous()
            if dn is not None:
                y = dn(y)
            y = y[0].cpu().numpy()
            x = np.load(tmp_path / "audios" / ("u%d-audio.npy" % k))[:n]
            assert r["samples"] == n and r["frames"] == 1 + n // hop and np.isfinite(y).all() and np.abs(y).max() > 0
            own, wide = R.dist(x, y, 64, 16, hp, fb), R.dist(x, y, 128, 32)
            b_own, b_wide = R.bound(x, y, 64, 16, hp, fb), R.bound(x, y, 128, 32)
            sh = [abs(r["mel_l1"] - own[0]) / b_own[0], abs(r["lsd_db@64/16"] - own[1]) / b_own[1], abs(r["sc@64/16"] - own[2]) / b_own[2],
                  abs(r["lsd_db@128/32"] - wide[1]) / b_wide[1], abs(r["sc@128/32"] - wide[2]) / b_wide[2]]
            print("%s u%d: %s of the bound" % (tag, k, " / ".join("%.4f" % s for s in sh)))
            assert max(sh) <= 1.0, (tag, k, r, own, wide)
            assert r["lsd_db"] == (r["lsd_db@64/16"] + r["lsd_db@128/32"]) / 2 and r["sc"] == (r["sc@64/16"] + r["sc@128/32"]) / 2
        s = np.float64(0.0)
        for r in out:
            s = s + np.float64(r["sc"])
        assert summary["sc"] == float(s / 4) and summary["measured/mel_l1"] == 4


def test_evaluate_two_directories_with_a_48_khz_file(tmp_path):
    hp = small_hparams(n_fft=64, sample_rate=16000, fmin=50, fmax=7600)
    fb = P.mel_filterbank(hp)
    ref, test = tmp_path / "ref", tmp_path / "test"
    ref.mkdir(), test.mkdir()
    t48 = np.arange(3 * 6000) / 48000.0
    tone48 = (0.4 * np.sin(2 * np.pi * 300.0 * t48) + 0.2 * np.sin(2 * np.pi * 1700.0 * t48)).astype(np.float32)
    t16 = np.arange(6100) / 16000.0
    tone16 = (0.4 * np.sin(2 * np.pi * 300.0 * t16) + 0.2 * np.sin(2 * np.pi * 1700.0 * t16)).astype(np.float32)
    _write_wav(ref / "tone.wav", tone48, 48000)                # the same tones at another rate: 6000 samples at 16 kHz
    _write_wav(test / "tone.wav", tone16, 16000)
    a, b = R.pair(5, 3000)
    _write_wav(ref / "noise.wav", a, 16000)
    _write_wav(test / "noise.wav", b[:2500], 16000)
    _write_wav(ref / "alone.wav", a, 16000)
    args = E.parse_args(["--ref_dir", str(ref), "--test_dir", str(test), "--out", str(tmp_path / "e.jsonl")])
    out, summary = E.evaluate_dirs(args, hp, device=DEV)
    assert [r["name"] for r in out] == ["noise.wav", "tone.wav"] and summary["only_in_ref_dir"] == ["alone.wav"]
    assert summary["only_in_test_dir"] == [] and [json.loads(s) for s in open(tmp_path / "e.jsonl")] == out + [summary]
    for r in out:
        x = P.load_wav(str(ref / r["name"]), hp.sample_rate)
        y = P.load_wav(str(test / r["name"]), hp.sample_rate)
        n = min(len(x), len(y))
        assert r["samples"] == n == (2500 if r["name"] == "noise.wav" else 6000)
        want, bd = R.dist(x[:n], y[:n], 64, 16, hp, fb), R.bound(x[:n], y[:n], 64, 16, hp, fb)
        assert max(R.shares((r["mel_l1"], r["lsd_db"], r["sc"]), want, bd)) <= 1.0 and r["frames"] == 1 + n // 16
    assert out[1]["sc"] < out[0]["sc"]                          # the resampled tone is nearer its 16 kHz twin than the noise pair is


def test_train_eval_metrics_writes_its_record_and_nothing_else_changes(tmp_path):
    from tf_flowavenet_amd import train as TL
    hp = small_hparams(n_block=3, n_flow=2, n_layer=2, hop_size=16, upsample_scales=[4, 4], num_mels=16, n_fft=64, sample_rate=8000,
                       fmin=50, fmax=3800, max_time_steps=256, batch_size=4, test_size=2, eval_max_time_steps=512)
    fb = P.mel_filterbank(hp)
    for tag in ("off", "on"):
        _corpus(str(tmp_path / tag / "training_data"), hp, [40, 57, 48, 33, 60, 45], seed=3)
        args = SimpleNamespace(base_dir=str(tmp_path / tag), restore=False, summary_interval=2, checkpoint_interval=100, eval_interval=2,
                               train_steps=2, seed=3, eval_metrics=(tag == "on"))
        TL.train(str(tmp_path / tag / "logs"), args, hp, "training_data/train.txt")
    on, off = tmp_path / "on" / "logs", tmp_path / "off" / "logs"
    assert not (off / "eval").exists() and sorted(os.listdir(on)) == sorted(os.listdir(off) + ["eval"])
    for sub, name in (("train", "summary.jsonl"), ("test", "summary.jsonl"), ("train", "predictions-2.wav"), ("train", "targets-2.wav")):
        assert (on / sub / name).read_bytes() == (off / sub / name).read_bytes(), name
    assert sorted(os.listdir(on / "train")) == sorted(os.listdir(off / "train"))
    ck_on, ck_off = (np.load(d / "pretrained" / "flowavenet_model.ckpt-2.npz") for d in (on, off))
    assert sorted(ck_on.files) == sorted(ck_off.files) and all(np.array_equal(ck_on[k], ck_off[k]) for k in ck_on.files)
    recs = [json.loads(s) for s in open(on / "eval" / "summary.jsonl")]
    assert len(recs) == 1 and set(recs[0]) == {"step", "eval/mel_l1", "eval/lsd_db", "eval/sc"} and recs[0]["step"] == 2
    assert all(np.isfinite(recs[0][k]) and recs[0][k] > 0 for k in recs[0])
