"""CPU tests of the spectral denoiser: the fp64 restatement (tests/denoise_ref.py) against scipy and against the properties
DESIGN.md 6b promises, the argument checks of ``Denoiser`` and of ``--denoise``, the CLI's paths with the restatement standing
in for the kernel, and the packed-fp32 check over the new unit's ISA."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import denoise_ref as R
from conftest import small_hparams
from tf_flowavenet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 8), (64, 16), (64, 32), (512, 96), (1024, 256)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _lengths(n_fft, hop):
    return [n_fft // 2 + 1, n_fft // 2 + 2, 5 * hop, 5 * hop + 1, 1000, 1001, 3 * 1024 + 1]


# ---- the restatement ----

def test_analysis_equals_scipy_stft_of_the_reflect_padded_signal():
    from scipy.signal import stft
    for n_fft, hop, n in ((64, 16, 1000), (512, 96, 3000), (32, 8, 17)):
        x = np.random.default_rng(n).uniform(-1.0, 1.0, n)
        w = R.hann(n_fft)
        padded = np.pad(x, n_fft // 2, mode="reflect")
        _, _, Z = stft(padded, window=w, nperseg=n_fft, noverlap=n_fft - hop, boundary=None, padded=False)
        X = R.stft(x, n_fft, hop)
        assert Z.shape[1] >= X.shape[0] - 1                    # scipy drops a last frame that does not fit whole
        f = min(Z.shape[1], X.shape[0])
        err = float(np.abs(X[:f] - Z.T[:f] * w.sum()).max())
        print("n_fft %d hop %d N %d: max |restatement - scipy| = %.2e over %d frames" % (n_fft, hop, n, err, f))
        assert f >= X.shape[0] - 1 and err <= 1e-12


@pytest.mark.parametrize("n_fft,hop", SHAPES)
def test_strength_zero_is_the_identity(n_fft, hop):
    rng = np.random.default_rng(n_fft + hop)
    bias = rng.uniform(0.0, 5.0, n_fft // 2 + 1)
    for n in _lengths(n_fft, hop):
        if n < n_fft // 2 + 1:
            continue
        x = rng.uniform(-1.0, 1.0, n)
        env = R.envelope(n, n_fft, hop)
        assert env.min() > 0.3                                 # hop <= n_fft / 2: every sample is covered
        err = float(np.abs(R.denoise(x, bias, 0.0, n_fft, hop) - x).max())
        assert err <= 1e-12, (n, err)


def test_a_clip_too_short_to_reflect_comes_back_unchanged():
    for n_fft, hop in SHAPES:
        x = np.random.default_rng(1).uniform(-1.0, 1.0, n_fft // 2)
        y = R.denoise(x, np.ones(n_fft // 2 + 1), 1.0, n_fft, hop)
        assert np.array_equal(y, x) and y is not x


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (512, 96), (1024, 256)])
def test_stationary_tones_are_removed_by_their_own_bias(n_fft, hop):
    n = 12 * n_fft + 37
    t = np.arange(n)
    x = sum(a * np.cos(2.0 * np.pi * k * t / n_fft + ph) for a, k, ph in ((0.4, 3, 0.3), (0.25, n_fft // 8, 1.1), (0.1, n_fft // 2 - 2, 2.0)))
    bias = R.mean_mag(x, n_fft, hop) * (1.0 + 1e-12)           # the interior frames all have this magnitude, to rounding
    y = R.denoise(x, bias, 1.0, n_fft, hop)
    peak = np.abs(x).max()
    inner = np.abs(y[n_fft:n - n_fft]).max()
    print("n_fft %d hop %d: residue %.2e of the peak" % (n_fft, hop, inner / peak))
    assert inner <= 1e-9 * peak
    assert np.abs(y[:n_fft]).max() > 1e-3 * peak               # the reflected ends are not stationary: something is left there
    assert np.abs(R.denoise(x, bias, 0.0, n_fft, hop) - x).max() <= 1e-12


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (512, 96)])
def test_an_output_depends_on_the_samples_within_n_fft_of_it(n_fft, hop):
    rng = np.random.default_rng(7)
    n = 10 * n_fft + 3
    x = rng.uniform(-1.0, 1.0, n)
    bias = rng.uniform(0.0, 3.0, n_fft // 2 + 1)
    y = R.denoise(x, bias, 0.5, n_fft, hop)
    i = 5 * n_fft + 11
    z = x.copy()
    z[:i - n_fft] = rng.uniform(-1.0, 1.0, i - n_fft)
    z[i + n_fft + 1:] = rng.uniform(-1.0, 1.0, n - i - n_fft - 1)
    y2 = R.denoise(z, bias, 0.5, n_fft, hop)
    assert y2[i] == y[i]
    assert np.abs(y2 - y).max() > 1e-3


def test_the_float32_run_of_the_restatement_sits_far_inside_the_bounds():
    """What the GPU tests' bounds are worth: float32 NumPy is at a few per cent of them, so an indexing, window or scaling
    error cannot hide inside, and a correct float32 kernel fits."""
    u = 2.0 ** -24
    for n_fft, hop in SHAPES:
        rng = np.random.default_rng(n_fft)
        x = np.clip(rng.normal(0.0, 0.3, 7 * hop + 5 + n_fft), -1.0, 1.0).astype(np.float32)
        bias = (rng.uniform(0.0, 1.0, n_fft // 2 + 1) * 0.1 * np.sqrt(n_fft)).astype(np.float32)
        ref = R.denoise(x.astype(np.float64), bias.astype(np.float64), 0.5, n_fft, hop)
        got = R.denoise(x, bias, 0.5, n_fft, hop)
        assert got.dtype == np.float32
        S, env, V = R.sample_bound_terms(x, n_fft, hop)
        per_sample = (16 * np.log2(n_fft) + 16) * u * S / env + 4 * u * np.abs(ref)
        per_clip = (16 * np.log2(n_fft) + 6) * u * np.sqrt((V ** 2).sum() / env.min()) + 4 * u * np.linalg.norm(ref)
        a, b = float((np.abs(got - ref) / per_sample).max()), float(np.linalg.norm(got - ref) / per_clip)
        print("n_fft %d hop %d: float32 NumPy at %.4f of the per-sample and %.4f of the per-clip bound" % (n_fft, hop, a, b))
        assert a <= 0.1 and b <= 0.1


# ---- argument checks ----

def test_denoiser_argument_checks(lib):
    from tf_flowavenet_amd.denoise import Denoiser, check_shape, check_strength
    ok = np.ones(33, dtype=np.float32)
    d = Denoiser(bias=ok, n_fft=64, hop=16, strength=0.0, device="cpu")
    assert (d.n_fft, d.hop, d.nb, d.strength) == (64, 16, 33, 0.0) and d.bias.shape == (33,)
    with pytest.raises(ValueError, match="either"):
        Denoiser()
    with pytest.raises(ValueError, match="either"):
        Denoiser(model=object(), bias=ok)
    with pytest.raises(ValueError, match="n_fft= and hop="):
        Denoiser(bias=ok, device="cpu")
    for bad in (np.ones(32), np.ones((1, 33)), -ok, ok * np.nan, ok * np.inf):
        with pytest.raises(ValueError, match="bias"):
            Denoiser(bias=bad, n_fft=64, hop=16, device="cpu")
    for n_fft, hop in ((16, 4), (48, 8), (8192, 64), (64, 0), (64, 33)):
        with pytest.raises(ValueError):
            check_shape(n_fft, hop)
    assert check_shape(4096, 2048) == (4096, 2048) and check_shape(32, 1) == (32, 1)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            check_strength(bad)
        with pytest.raises(ValueError, match="strength"):
            Denoiser(bias=ok, n_fft=64, hop=16, strength=bad, device="cpu")
        with pytest.raises(ValueError, match="strength"):
            d(np.zeros(100, dtype=np.float32), strength=bad)


def test_c_entries_refuse_without_a_device(lib):
    P = 1 << 20
    assert lib.fwn_denoise(P, 1, 1000, None, 1000, P, 0.5, 100, 16, P + (1 << 16), 1000, None, 0, None, 0, None) == -1
    assert b"fwn_denoise" in lib.fwn_last_error() and b"power of two" in lib.fwn_last_error()
    assert lib.fwn_denoise(P, 1, 1000, None, 1000, P, -1.0, 64, 16, P + (1 << 16), 1000, None, 0, None, 0, None) == -1
    assert b"strength" in lib.fwn_last_error()
    assert lib.fwn_stft_mean_mag(P, 1, 1000, 40, 64, 16, P + (1 << 16), None) == -1 and b"no interior frame" in lib.fwn_last_error()
    assert lib.fwn_denoise_workspace_bytes(1, 1 << 34, 1024, 256) == 0         # the fused form: nothing proportional to the clip
    assert lib.fwn_denoise_tile(1024, 256) >= 256


def test_denoise_flag_parses_and_bad_strengths_are_parser_errors(monkeypatch, capsys):
    from tf_flowavenet_amd import synthesize as S
    seen = []
    monkeypatch.setattr(S, "synthesize", lambda args, hp: seen.append(vars(args)))
    S.main([])
    S.main(["--denoise", "0.05", "--device_rng", "--ragged"])
    S.main(["--denoise", "0"])
    assert "denoise" not in seen[0]                            # off by default: the namespace is what it was
    assert seen[1]["denoise"] == 0.05 and seen[1]["device_rng"] is True and seen[2]["denoise"] == 0.0
    for bad in ("-0.1", "nan", "inf", "loud"):
        with pytest.raises(SystemExit) as e:
            S.main(["--denoise=" + bad])
        assert e.value.code == 2 and "--denoise" in capsys.readouterr().err
    assert len(seen) == 3


# ---- the CLI's paths, the restatement standing in for the kernel ----

BIAS = np.linspace(0.5, 0.05, 33)
CLIPS = [("a", 5), ("b", 3), ("c", 5), ("d", 9)]           # mel frames; n_block 5 at hop 16: odd counts are edge-padded by a frame


def _stub(monkeypatch, events):
    import torch
    from tf_flowavenet_amd import denoise as DN
    from tf_flowavenet_amd import resample as RS

    class FakeDenoiser:
        def __init__(self, model, strength=0.01):
            self.strength = strength

        def __call__(self, x, lengths=None, pcm=False, strength=None):
            x = x.numpy()
            one = x.ndim == 1
            x = x[None] if one else x
            lengths = [x.shape[1]] * len(x) if lengths is None else list(lengths)
            out = np.zeros(x.shape)
            for b, n in enumerate(lengths):
                out[b, :n] = R.denoise(x[b, :n].astype(np.float64), BIAS, self.strength, 64, 16)
            out = R.pcm16(out) if pcm else out.astype(np.float32)
            events.append(("denoise", lengths, x.shape, pcm, out.copy()))
            return torch.from_numpy(out[0] if one else out)

    class FakeResampler:
        def __init__(self, in_rate, out_rate):
            pass

        def out_length(self, n):
            return n // 2

        def __call__(self, x, lengths=None):
            events.append(("resample", None if lengths is None else list(lengths), x.numpy().copy()))
            return x[..., ::2]

    class Event:
        def record(self):
            pass

        def synchronize(self):
            pass

    monkeypatch.setattr(DN, "Denoiser", FakeDenoiser)
    monkeypatch.setattr(RS, "Resampler", FakeResampler)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)          # no device here: the model below is a stand-in
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "Event", Event)


class _Model:
    """A stand-in for FloWaveNet: audio that is a fixed function of the mel, so every path 'synthesizes' the same clip."""
    hop = 16

    def __init__(self, hp):
        self._hparams = hp

    @staticmethod
    def _audio(c):
        import torch
        c = torch.as_tensor(c)
        t = torch.arange(c.shape[1] * 16, dtype=torch.float32)
        return (0.6 * torch.sin(0.37 * t)[None] * (0.5 + c[:, :, 0].repeat_interleave(16, dim=1)))[:, :, None]

    def reverse(self, z, c, lengths=None):
        return self._audio(c)

    def reverse_windowed(self, z, c, window, batch=8):
        return self._audio(c)

    def synthesize(self, c, seed, clip_ids=None, lengths=None, return_wav=False):
        import torch
        wav = self._audio(c)
        pcm = torch.from_numpy(R.pcm16(wav[:, :, 0].numpy()))
        return (pcm, wav) if return_wav else pcm

    def synthesize_windowed(self, c, seed, clip_ids=None, window=None, batch=8, return_wav=False):
        return self.synthesize(c, seed, return_wav=return_wav)


def _case(tmp_path):
    hp = small_hparams(n_block=5, n_fft=64)
    (tmp_path / "mels").mkdir()
    rng = np.random.default_rng(0)
    mels = {}
    for name, frames in CLIPS:
        mels[name] = rng.random((frames, hp.num_mels), dtype=np.float32)
        np.save(tmp_path / "mels" / (name + ".npy"), mels[name])
    return hp, mels


def _read(path):
    with wave.open(str(path)) as w:
        return w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("path", ["default", "ragged", "device", "device_ragged", "window", "window_device"])
def test_every_cli_path_hands_the_denoiser_the_true_samples(monkeypatch, tmp_path, path):
    from tf_flowavenet_amd import synthesize as S
    events = []
    _stub(monkeypatch, events)
    hp, mels = _case(tmp_path)
    extra = {"default": {}, "ragged": dict(ragged=True, max_pad_frac=0.5), "device": dict(device_rng=True),
             "device_ragged": dict(device_rng=True, ragged=True, max_pad_frac=0.5), "window": dict(window=100),
             "window_device": dict(window=100, device_rng=True)}[path]
    args = type("A", (), dict(mels_dir=str(tmp_path / "mels"), output_dir=str(tmp_path / "out"), seed=1, batch=4, denoise=0.5, **extra))()
    S.synthesize(args, hp, model=_Model(hp))
    calls = [e for e in events if e[0] == "denoise"]
    assert calls and len(calls) == len(events)
    given = sorted(n for e in calls for n in e[1])
    assert given == sorted(f * 16 for _, f in CLIPS)           # the true samples: frames * hop, not the edge-padded length
    assert all(e[3] == ("device" in path) for e in calls)      # int16 comes out of the denoiser on the device path, float elsewhere
    if path.startswith("window"):
        assert [9 * 16] in [e[1] for e in calls] and (1, 9 * 16) in [e[2] for e in calls]    # d (144 > 128 samples): whole, alone
    for name, frames in CLIPS:
        n = frames * 16
        x = _Model._audio(mels[name][None])[0, :, 0].numpy().astype(np.float64)
        want = R.pcm16(R.denoise(x, BIAS, 0.5, 64, 16))
        rate, got = _read(tmp_path / "out" / (name + ".wav"))
        assert rate == hp.sample_rate and len(got) == n and np.array_equal(got, want), name


@pytest.mark.parametrize("path", ["default", "ragged", "window"])
def test_out_rate_runs_after_the_denoiser_on_its_output(monkeypatch, tmp_path, path):
    from tf_flowavenet_amd import synthesize as S
    events = []
    _stub(monkeypatch, events)
    hp, mels = _case(tmp_path)
    extra = {"default": {}, "ragged": dict(ragged=True, max_pad_frac=0.5), "window": dict(window=100)}[path]
    args = type("A", (), dict(mels_dir=str(tmp_path / "mels"), output_dir=str(tmp_path / "out"), seed=1, batch=4, denoise=0.5,
                              out_rate=11025, **extra))()
    S.synthesize(args, hp, model=_Model(hp))
    kinds = [e[0] for e in events]
    assert kinds == ["denoise", "resample"] * (len(kinds) // 2) and kinds
    for dn, rs in zip(events[0::2], events[1::2]):
        assert np.array_equal(np.squeeze(rs[2]), np.squeeze(dn[4]))            # the resampler's input is the denoiser's output
        assert rs[1] is None or rs[1] == dn[1]                                 # and the same true lengths
    for name, frames in CLIPS:
        rate, got = _read(tmp_path / "out" / (name + ".wav"))
        assert rate == 11025 and len(got) == frames * 16 // 2


def test_without_the_flag_no_denoiser_is_built(monkeypatch, tmp_path):
    from tf_flowavenet_amd import denoise as DN
    from tf_flowavenet_amd import synthesize as S
    events = []
    _stub(monkeypatch, events)

    def boom(*a, **k):
        raise AssertionError("denoiser reached without --denoise")

    monkeypatch.setattr(DN, "Denoiser", boom)
    hp, mels = _case(tmp_path)
    for extra in ({}, dict(ragged=True, max_pad_frac=0.5), dict(device_rng=True), dict(window=100), dict(window=100, device_rng=True)):
        args = type("A", (), dict(mels_dir=str(tmp_path / "mels"), output_dir=str(tmp_path / "out"), seed=1, batch=4, **extra))()
        S.synthesize(args, hp, model=_Model(hp))
        for name, frames in CLIPS:
            x = _Model._audio(mels[name][None])[0, :, 0].numpy()
            assert np.array_equal(_read(tmp_path / "out" / (name + ".wav"))[1], R.pcm16(x)), (extra, name)
    assert not events


# ---- the new unit's ISA ----

@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_swizzled_packed_fp32_in_the_denoise_unit(tmp_path):
    """tools/check_packed_f32.py (tests/test_static_isa.py has the story) over csrc/denoise.hip, built with the Makefile's flags."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_packed_f32 as chk
    csrc = os.path.join(ROOT, "tf-flowavenet_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    assert "denoise.hip" in re.search(r"^SRCS\s*=\s*(.*)$", text, re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(EXTRA)", "").replace("$(ARCH)", arch).split()
    assert "-fno-slp-vectorize" in flags and "--offload-arch=gfx950" in flags
    out = tmp_path / "denoise.s"
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-c", os.path.join(csrc, "denoise.hip"), "-o", str(out)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ks = list(chk.kernels(str(out)))
    assert sorted(("denoise_kernel" in name) + 2 * ("mean_mag_kernel" in name) for name, _ in ks) == [1, 2], [name for name, _ in ks]
    flagged = [(name, rep[:2]) for name, body in ks for rep in [chk.check(name, body)] if rep]
    assert not flagged, flagged[:3]
