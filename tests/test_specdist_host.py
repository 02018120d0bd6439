"""CPU tests of the spectral distances: the restatement (tests/specdist_ref.py) against scipy and against the mel
front-end's restatement, its known answers in fp64, what its bound is worth, every refusal of the C entry point - before any
launch: there is no device here -, and the ``evaluate`` CLI and the training hook's record over a NumPy compute step."""
import json
import os
import wave

import numpy as np
import pytest

import mel_front_ref as MR
import specdist_ref as R
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import evaluate as E
from tf_flowavenet_amd import metrics as M
from tf_flowavenet_amd import preprocessing as P


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- the restatement ----
@pytest.mark.parametrize("n_fft,hop,n_mels", R.SHAPES)
def test_analysis_is_scipys_stft_of_the_reflect_padded_signal(n_fft, hop, n_mels):
    from scipy.signal import stft
    n = 3 * R.FRAMES * hop
    x = MR.signal(n_fft, n)
    xp = np.pad(x.astype(np.float64), n_fft // 2, mode="reflect")
    _, _, Z = stft(xp, window="hann", nperseg=n_fft, noverlap=n_fft - hop, boundary=None, padded=False, return_onesided=True)
    Z = Z.T * np.hanning(n_fft + 1)[:-1].sum()                 # scipy scales by 1 / sum(window)
    p = R.power64(x, n_fft, hop)
    assert p.shape == (1 + n // hop, n_fft // 2 + 1) == Z.shape
    assert np.abs(p - np.abs(Z) ** 2).max() <= 1e-10 * p.max()


@pytest.mark.parametrize("n_fft,hop,n_mels,n", MR.SHAPES)
def test_mel_is_the_front_ends(n_fft, hop, n_mels, n):
    """The oracle's filterbank is fp64, the device's its float32 rounding: 2^-24 relative on a power, 20 log10(e) 2^-24 / 100 on
    a mel - the restatement over the oracle's own table agrees to fp64 rounding."""
    from oracle import mel_np as onp
    hp = MR.hp_of(n_fft, hop, n_mels)
    x = MR.signal(n, n)
    m0 = MR.front(x, hp, normalize=False)[1]
    fb64 = onp.mel_filterbank(hp.sample_rate, hp.n_fft, hp.num_mels, hp.fmin, hp.fmax)
    assert np.abs(R.mel64(x, hp, fb64) - m0).max() <= 1e-9 and np.abs(MR.mel64(x, hp) - m0).max() <= 1e-9
    assert np.abs(R.mel64(x, hp, P.mel_filterbank(hp)) - m0).max() <= 20 * np.log10(np.e) * 2.0 ** -24 / 100 + 1e-9


# ---- known answers in fp64 ----
def _noise(seed, n):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("n_fft,hop,n_mels,n", [(256, 100, 20, 901), (512, 128, 40, 1300), (1024, 256, 80, 1500)])
def test_known_answers(n_fft, hop, n_mels, n):
    """y = 0.5 x quarters every power: each level difference is 10 log10 4 = 20 log10 2 dB, and each mel - ``fwn_mel_front``'s
    20 log10 of a POWER over -min_level_db, kept from the reference - moves by 20 log10 4 / -min_level_db, i.e. twice
    20 log10 2 / -min_level_db (the figure of a 20 log10 |X| mel; this front-end's is 20 log10 |X|^2)."""
    hp = MR.hp_of(n_fft, hop, n_mels)
    fb = P.mel_filterbank(hp)
    def plain(s):                                              # every bin of 0.5 x above the floor, every mel of it above its clip
        half = np.float32(0.5) * _noise(s, n)
        return R.power64(half, n_fft, hop).min() > R.FLOOR and R.mel64(half, hp, fb).min() > 0.0
    seed = next(s for s in range(100) if plain(s))
    x = _noise(seed, n)
    y = (np.float32(0.5) * x).astype(np.float32)               # exact in float32
    assert R.power64(y, n_fft, hop).min() > R.FLOOR             # every bin of both clips above the floor
    for c in (x, y):
        m = R.mel64(c, hp, fb)
        assert 0.0 < m.min() and m.max() < 1.0                 # no mel clipped
    assert R.dist(x, x, n_fft, hop, hp, fb) == (0.0, 0.0, 0.0, 1 + n // hop)
    mel, lsd, sc, frames = R.dist(x, y, n_fft, hop, hp, fb)
    assert abs(sc - 0.5) <= 1e-12 and abs(lsd - 20 * np.log10(2.0)) <= 1e-12
    assert abs(mel - 2 * 20 * np.log10(2.0) / -hp.min_level_db) <= 1e-12 and frames == 1 + n // hop
    mel, lsd, sc, _ = R.dist(x, np.zeros_like(x), n_fft, hop, hp, fb)
    assert abs(sc - 1.0) <= 1e-12 and lsd > 0 and mel > 0
    _, lsd, sc, _ = R.dist(np.zeros_like(x), x, n_fft, hop)     # a silent target: the IEEE quotient, x / 0
    assert sc == float("inf") and lsd > 0
    assert np.isnan(R.dist(np.zeros_like(x), np.zeros_like(x), n_fft, hop)[2])
    short = R.dist(x[:n_fft // 2], y[:n_fft // 2], n_fft, hop, hp, fb)
    assert all(np.isnan(v) for v in short[:3]) and short[3] == 0
    assert not np.isnan(R.dist(x[:n_fft // 2 + 1], y[:n_fft // 2 + 1], n_fft, hop, hp, fb)[:3]).any()


# ---- the error bound ----
@pytest.mark.parametrize("n_fft,hop,n_mels", R.SHAPES)
def test_float32_numpy_sits_inside_the_bound(n_fft, hop, n_mels):
    hp = MR.hp_of(n_fft, hop, n_mels)
    fb = P.mel_filterbank(hp)
    worst = [0.0, 0.0, 0.0]
    for n in R.lengths_of(n_fft, hop):
        x, y = R.pair(n, n)
        ref, bd = R.dist(x, y, n_fft, hop, hp, fb), R.bound(x, y, n_fft, hop, hp, fb)
        sh = R.shares(R.dist32(x, y, n_fft, hop, hp, fb), ref, bd)
        worst = [max(a, b) for a, b in zip(worst, sh)]
        assert all(b > 0 for b in bd) and bd[0] <= 2e-4 and bd[1] <= 1e-2 and bd[2] <= 1e-4        # the bound is worth something
        assert max(sh) <= 1.0, (n, sh)
    print("n_fft %d hop %d n_mels %d: float32 NumPy at %.4f / %.4f / %.4f of the bound (mel_l1 / lsd_db / sc)" % ((n_fft, hop, n_mels) + tuple(worst)))


# ---- the C entry: every refusal, without a device ----
def test_c_entry_refuses_without_a_device(lib):
    for kw, word in R.REFUSALS:
        assert R.refusal_call(lib, **kw) == -1, kw
        msg = lib.fwn_last_error()
        assert b"fwn_spectral_distance" in msg and word in msg, (kw, msg)
    assert lib.fwn_spectral_distance_frames(100, 16) == -1 and b"fwn_spectral_distance_frames" in lib.fwn_last_error()
    assert lib.fwn_spectral_distance_frames(64, 40) == -1
    for n_fft, hop, _ in R.SHAPES:
        assert lib.fwn_spectral_distance_frames(n_fft, hop) == R.FRAMES
    assert lib.fwn_spectral_distance_workspace_bytes(2, 1000, 64, 16) == 2 * 8 * 32
    assert lib.fwn_spectral_distance_workspace_bytes(3, 127, 32, 16) == 3 * 1 * 32
    assert lib.fwn_spectral_distance_workspace_bytes(3, 128, 32, 16) == 3 * 2 * 32
    assert lib.fwn_spectral_distance_workspace_bytes(0, 1000, 64, 16) == 0 and lib.fwn_spectral_distance_workspace_bytes(1, 1000, 60, 16) == 0


def test_unit_is_in_the_build():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "tf-flowavenet_amd", "csrc", "Makefile")).read()
    assert "specdist.hip" in re.search(r"^SRCS\s*=\s*(.*)$", text, re.M).group(1).split()
    assert re.search(r"^specdist\.o:.*stft_lds\.h", text, re.M)


# ---- the Python surface and the CLI, over a NumPy compute step ----
def test_resolution_arg_and_combine():
    assert M.resolution_arg("512/128,1024/256,2048/512") == [(512, 128), (1024, 256), (2048, 512)]
    for bad in ("512", "500/100", "512/300", "a/b"):
        with pytest.raises(ValueError):
            M.resolution_arg(bad)
    a = np.array([[0.1, 2.0, 0.2, 9.0]])
    b = np.array([[np.nan, 4.0, 0.4, 5.0]])
    d = M.combine([b, a], a, [(64, 8), (128, 16)])
    assert d["mel_l1"][0] == 0.1 and d["frames"][0] == 9.0 and d["lsd_db"][0] == 3.0 and abs(d["sc"][0] - 0.3) < 1e-15
    assert d["lsd_db@64/8"][0] == 4.0 and d["sc@128/16"][0] == 0.2 and len(d) == 8


def _write_wav(path, x, rate):
    pcm = (np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def _hp():
    from conftest import small_hparams
    return small_hparams(n_fft=64)


def test_two_directories_pairing_cropping_and_summary(tmp_path):
    hp = _hp()
    ref, test = tmp_path / "a", tmp_path / "b"
    ref.mkdir(), test.mkdir()
    clips = {"u1.wav": (700, 650), "u2.wav": (400, 400), "u3.wav": (2000, 2100), "u4.wav": (20, 900), "u5.wav": (660, 700)}
    for k, (name, (na, nb)) in enumerate(sorted(clips.items())):
        x, y = R.pair(k, max(na, nb))
        _write_wav(ref / name, x[:na], hp.sample_rate)
        _write_wav(test / name, y[:nb], hp.sample_rate)
    _write_wav(ref / "only_ref.wav", MR.signal(1, 300), hp.sample_rate)
    _write_wav(test / "only_test.wav", MR.signal(2, 300), hp.sample_rate)
    (test / "notes.txt").write_text("not a wav")
    res = [(64, 16), (128, 32)]
    metric = R.NumpyMetric(hp, res)
    args = E.parse_args(["--ref_dir", str(ref), "--test_dir", str(test), "--out", str(tmp_path / "e.jsonl"), "--batch", "3",
                         "--resolutions", "64/16,128/32"])
    assert args.resolutions == res
    out, summary = E.evaluate_dirs(args, hp, metric=metric, device="cpu")
    lines = [json.loads(s) for s in open(tmp_path / "e.jsonl")]
    assert lines[:-1] == out and lines[-1] == summary and [r["name"] for r in out] == sorted(clips)
    assert summary["summary"] is True and summary["utterances"] == 5
    assert summary["only_in_ref_dir"] == ["only_ref.wav"] and summary["only_in_test_dir"] == ["only_test.wav"]
    fb = P.mel_filterbank(hp)
    for r in out:
        n = min(clips[r["name"]])
        a = P.load_wav(str(ref / r["name"]), hp.sample_rate)[:n]
        b = P.load_wav(str(test / r["name"]), hp.sample_rate)[:n]
        assert r["samples"] == n
        if r["name"] == "u4.wav":                              # 20 samples: too short to frame at either resolution
            assert r["frames"] == 0 and r["mel_l1"] is None and r["lsd_db"] is None and r["sc@128/32"] is None
            continue
        own, wide = R.dist32(a, b, 64, 16, hp, fb), R.dist32(a, b, 128, 32)
        assert r["frames"] == 1 + n // 16 and r["mel_l1"] == own[0]
        assert r["lsd_db@64/16"] == own[1] and r["sc@128/32"] == wide[2]
        assert r["lsd_db"] == (own[1] + wide[1]) / 2.0 and r["sc"] == (own[2] + wide[2]) / 2.0
    live = [r for r in out if r["mel_l1"] is not None]
    for key in ("mel_l1", "lsd_db", "sc", "sc@64/16"):
        s = np.float64(0.0)
        for r in live:
            s = s + np.float64(r[key])
        assert summary[key] == float(s / 4) and summary["measured/" + key] == 4
    # batched by plan_batches: no call holds more than --batch rows, every live pair is in exactly one call, cropped
    assert all(shape[0] <= 3 and shape[1] == max(lens) for shape, lens in metric.calls)
    assert sorted(n for _, lens in metric.calls for n in lens) == sorted(min(v) for v in clips.values())


def test_training_hooks_record():
    hp = _hp()
    x, y = R.pair(3, 640)
    d = R.NumpyMetric(hp).dist(x, y)
    rec = E.eval_record(500, d)
    fb = P.mel_filterbank(hp)
    mel, lsd, sc, _ = R.dist32(x, y, 64, 16, hp, fb)
    assert rec == {"step": 500, "eval/mel_l1": mel, "eval/lsd_db": lsd, "eval/sc": sc}
    assert json.loads(json.dumps(rec)) == rec
    from tf_flowavenet_amd import train as T
    import inspect
    assert "--eval_metrics" in inspect.getsource(T.main)


def test_both_parser_errors(capsys):
    for bad in (["--saved_dir", "s/", "--base_dir", "d/", "--ref_dir", "a/", "--test_dir", "b/"],
                ["--ref_dir", "a/", "--test_dir", "b/", "--base_dir", "d/"]):
        with pytest.raises(SystemExit) as e:
            E.parse_args(bad)
        assert e.value.code == 2 and "not both" in capsys.readouterr().err
    for bad in ([], ["--ref_dir", "a/"], ["--saved_dir", "s/"]):
        with pytest.raises(SystemExit) as e:
            E.parse_args(bad)
        assert e.value.code == 2 and "--ref_dir and --test_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        E.parse_args(["--ref_dir", "a/", "--test_dir", "b/", "--denoise", "0.1"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        E.parse_args(["--ref_dir", "a/", "--test_dir", "b/", "--resolutions", "500/100"])
    assert "--resolutions" in capsys.readouterr().err
    a = E.parse_args(["--saved_dir", "s/", "--base_dir", "d/", "--denoise", "0.02", "--window", "4096"])
    assert a.denoise == 0.02 and a.window == 4096 and a.resolutions is None and a.ref_dir is None
