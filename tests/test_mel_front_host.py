"""CPU tests of the ragged mel front-end: the restatement (tests/mel_front_ref.py) against the oracle, what its bound is worth,
the ``bands`` table, ``MelStream``'s planning over a NumPy compute step, the parser rules of ``--wavs_dir`` and ``--batch``,
and every refusal of the two C entry points - all before any launch."""
import os

import numpy as np
import pytest

import mel_front_ref as R
from oracle import mel_np as onp
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import preprocessing as P


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("n_fft,hop,n_mels,n", R.SHAPES)
def test_restatement_agrees_with_the_oracle(n_fft, hop, n_mels, n):
    hp = R.hp_of(n_fft, hop, n_mels)
    x = R.signal(n, n)
    audio, mel, pk, xn = R.front(x, hp)
    a0, _ = onp.process_utterance(x, hp)
    assert audio.dtype == np.float32 and audio.shape == a0.shape == (R.frames_of(n, hop) * hop,)
    assert np.abs(audio - a0).max() <= 1e-6
    assert pk == np.abs(x).max() and np.abs(xn).max() == np.float32(hp.rescaling_max)
    assert np.array_equal(xn, (x / float(pk) * hp.rescaling_max))                    # _process_utterance's own line, bit for bit
    m0 = onp.melspectrogram(xn.astype(np.float64), hp)
    assert mel.shape == m0.shape == (R.frames_of(n, hop), n_mels)
    assert np.abs(mel - m0).max() <= 1e-9 and np.abs(R.mel64(xn, hp) - m0).max() <= 1e-9


def test_degenerate_clips_are_zeros_and_the_peak_tells():
    hp = R.hp_of(64, 16, 8)
    for x in (np.zeros(100, np.float32), np.r_[R.signal(1, 99), np.float32("nan")], R.signal(2, 32)):
        audio, mel, pk, _ = R.front(x, hp)
        assert not audio.any() and not mel.any() and mel.shape == (R.frames_of(len(x), 16), 8)
        assert len(x) == 32 or not pk > 0.0
    assert R.peak(np.zeros(0)) == 0.0 and np.isnan(R.peak([1.0, np.nan]))


@pytest.mark.parametrize("n_fft,hop,n_mels,n", R.SHAPES)
def test_float32_numpy_sits_inside_the_bound_and_the_bound_inside_the_suites_tolerance(n_fft, hop, n_mels, n):
    """What the GPU test's bound is worth: it is below the suite's mel tolerance (2e-4), so it asks more than test_mel.py does,
    and a float32 evaluation in NumPy uses a small part of it, so a correct float32 kernel fits."""
    hp = R.hp_of(n_fft, hop, n_mels)
    fb = P.mel_filterbank(hp)
    for seed in (3, 4):
        _, ref, _, xn = R.front(R.signal(seed + n, n), hp)
        bd = R.bound(xn, hp, fb)
        ratio = float((np.abs(R.mel32(xn, hp, fb) - ref) / bd).max())
        print("n_fft %d hop %d n_mels %d N %d seed %d: bound.max() %.2e, float32 NumPy at %.4f of the bound"
              % (n_fft, hop, n_mels, n, seed, bd.max(), ratio))
        assert bd.shape == ref.shape and bd.min() >= 32 * R.U
        assert bd.max() <= 2e-4
        assert ratio <= 1.0


def test_bands_cover_every_nonzero_entry():
    for n_fft, hop, n_mels, _ in R.SHAPES:
        fb = P.mel_filterbank(R.hp_of(n_fft, hop, n_mels))
        bands = P.mel_bands(fb)
        assert bands.dtype == np.int32 and bands.shape == (n_mels, 2)
        inside = (np.arange(fb.shape[1])[None] >= bands[:, :1]) & (np.arange(fb.shape[1])[None] < bands[:, 1:])
        assert not fb[~inside].any() and (bands >= 0).all() and (bands <= fb.shape[1]).all()
        for m, (lo, hi) in enumerate(bands):
            assert (lo == hi == 0 and not fb[m].any()) or (fb[m, lo] != 0 and fb[m, hi - 1] != 0)
    assert bands.sum() > 0


@pytest.mark.parametrize("step", [1, 7, 16, 333, 5000])
def test_melstream_planning_gives_the_whole_clips_frames_in_any_split(step):
    hp = R.hp_of(64, 16, 8)
    fb = P.mel_filterbank(hp)
    x = R.signal(5, 5000)
    whole = R.frame_mels32(x, hp, fb)
    calls = []

    def compute(samples):
        calls.append(len(samples))
        return R.frame_mels32(samples, hp, fb)

    s = P.MelStream(hp, compute=compute)
    parts, held = [], 0
    for a in range(0, len(x), step):
        out = s.push(x[a:a + step])
        held = max(held, s.retained)
        if out is not None:
            parts.append(out)
    parts.append(s.finish())
    got = np.concatenate(parts)
    assert got.shape == whole.shape == (1 + 5000 // 16, 8)
    assert np.array_equal(got, whole)
    assert held <= hp.n_fft + hp.hop_size + step and max(calls) <= hp.n_fft + 2 * hp.hop_size + step
    with pytest.raises(RuntimeError):
        s.push(x[:1])


def test_melstream_gain_and_short_clips():
    hp = R.hp_of(64, 16, 8)
    fb = P.mel_filterbank(hp)
    x = R.signal(6, 700)
    s = P.MelStream(hp, gain=0.5, compute=lambda v: R.frame_mels32(v, hp, fb))
    parts = [s.push(x[:300]), s.push(x[300:]), s.finish()]
    assert np.array_equal(np.concatenate([p for p in parts if p is not None]), R.frame_mels32(x * np.float32(0.5), hp, fb))
    for n in (0, 1, 32):
        s = P.MelStream(hp, compute=lambda v: R.frame_mels32(v, hp, fb))
        assert s.push(x[:n]) is None
        with pytest.raises(ValueError, match="reflect"):
            s.finish()
    s = P.MelStream(hp, compute=lambda v: R.frame_mels32(v, hp, fb))        # n_fft / 2 + 1 samples: the shortest clip there is
    first, rest = s.push(x[:33]), s.finish()
    assert len(first) == 1 and np.array_equal(np.concatenate([first, rest]), R.frame_mels32(x[:33], hp, fb))


def test_wavs_dir_and_batch_parser_rules(monkeypatch, capsys):
    from tf_flowavenet_amd import synthesize as S
    seen = []
    monkeypatch.setattr(S, "synthesize", lambda args, hp: seen.append(vars(args)))
    S.main([])
    S.main(["--wavs_dir", "w/", "--ragged"])
    S.main(["--mels_dir", "m/"])
    assert "wavs_dir" not in seen[0] and "_given" not in seen[0] and seen[0]["mels_dir"] == "mels/"
    assert seen[1]["wavs_dir"] == "w/" and seen[1]["ragged"] is True and "_given" not in seen[1]
    assert seen[2]["mels_dir"] == "m/" and "wavs_dir" not in seen[2] and "_given" not in seen[2]
    for bad in (["--wavs_dir", "w/", "--mels_dir", "m/"], ["--mels_dir=m/", "--wavs_dir=w/"]):
        with pytest.raises(SystemExit) as e:
            S.main(bad)
        assert e.value.code == 2 and "--wavs_dir" in capsys.readouterr().err
    assert len(seen) == 3
    assert "batch" not in vars(P.parse_args([])) and P.parse_args(["--batch", "4", "-i", "a"]).batch == 4
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit) as e:
            P.parse_args(["--batch", bad])
        assert e.value.code == 2 and "--batch" in capsys.readouterr().err


def _front(lib, **kw):
    """fwn_mel_front with plausible (never dereferenced) addresses, one argument changed: every refusal comes before any launch."""
    Q = 1 << 24
    a = dict(x=Q, B=2, x_stride=1000, len_dev=None, len_host=1000, peak=9 * Q, rmax=0.999, fb=10 * Q, bands=11 * Q, n_fft=64, hop=16,
             n_mels=8, ref=20.0, lo=-100.0, mel=2 * Q, mel_stride=63 * 8, audio=3 * Q, audio_stride=63 * 16)
    a.update(kw)
    return lib.fwn_mel_front(a["x"], a["B"], a["x_stride"], a["len_dev"], a["len_host"], a["peak"], a["rmax"], a["fb"], a["bands"],
                             a["n_fft"], a["hop"], a["n_mels"], a["ref"], a["lo"], a["mel"], a["mel_stride"], a["audio"],
                             a["audio_stride"], None)


def test_c_entries_refuse_without_a_device(lib):
    Q = 1 << 24
    cases = [(dict(n_fft=100), b"power of two"), (dict(n_fft=16), b"power of two"), (dict(n_fft=8192), b"power of two"),
             (dict(hop=0), b"hop"), (dict(hop=33), b"hop"),
             (dict(x=None), b"null"), (dict(fb=None), b"null"), (dict(mel=None), b"null"),
             (dict(x=Q + 2), b"alignment"), (dict(len_dev=Q + 4), b"alignment"), (dict(peak=Q + 1), b"alignment"),
             (dict(fb=Q + 2), b"alignment"), (dict(bands=Q + 2), b"alignment"), (dict(mel=Q + 3), b"alignment"),
             (dict(audio=Q + 1), b"alignment"),
             (dict(B=0), b"1..65535"), (dict(B=65536), b"1..65535"),
             (dict(len_host=0), b"2^40"), (dict(len_host=(1 << 40) + 1, x_stride=1 << 41), b"2^40"),
             (dict(x_stride=999), b"stride"), (dict(x_stride=(1 << 44) + 1), b"stride"),
             (dict(mel_stride=63 * 8 - 1), b"stride"), (dict(audio_stride=63 * 16 - 1), b"stride"),
             (dict(mel_stride=(1 << 44) + 1), b"stride"), (dict(audio_stride=(1 << 44) + 1), b"stride"),
             (dict(lo=0.0), b"min_level_db"), (dict(lo=5.0), b"min_level_db"), (dict(lo=float("nan")), b"min_level_db"),
             (dict(rmax=float("inf")), b"rmax"), (dict(rmax=float("nan")), b"rmax"), (dict(rmax=0.0), b"rmax"),
             (dict(rmax=-1.0), b"rmax"),
             (dict(n_mels=0), b"n_mels"), (dict(n_mels=1025), b"n_mels"),
             (dict(len_host=1 << 40, x_stride=1 << 40, hop=1, B=1, mel_stride=1 << 44, audio_stride=1 << 41), b"workgroups"),
             (dict(mel=Q + 4000), b"overlaps"), (dict(audio=Q + 7996), b"overlaps"), (dict(mel=Q - 4), b"overlaps")]
    for kw, word in cases:
        assert _front(lib, **kw) == -1, kw
        msg = lib.fwn_last_error()
        assert b"fwn_mel_front" in msg and word in msg, (kw, msg)
    peak_cases = [(dict(n=0), b"2^40"), (dict(B=0), b"1..65535"), (dict(B=1 << 16), b"1..65535"), (dict(x=None), b"null"),
                  (dict(out=None), b"null"), (dict(x=Q + 1), b"alignment"), (dict(out=Q * 2 + 2), b"alignment"),
                  (dict(len_dev=Q + 4), b"alignment"), (dict(stride=999), b"stride"), (dict(stride=(1 << 44) + 8), b"stride"),
                  (dict(n=(1 << 40) + 1, stride=1 << 41), b"2^40"), (dict(out=Q + 4004), b"overlaps")]
    for kw, word in peak_cases:
        a = dict(x=Q, B=2, stride=1000, len_dev=None, n=1000, out=2 * Q)
        a.update(kw)
        assert lib.fwn_clip_peak(a["x"], a["B"], a["stride"], a["len_dev"], a["n"], a["out"], None) == -1, kw
        msg = lib.fwn_last_error()
        assert b"fwn_clip_peak" in msg and word in msg, (kw, msg)
    assert lib.fwn_mel_front_frames(100, 16) == -1 and b"fwn_mel_front_frames" in lib.fwn_last_error()
    assert lib.fwn_mel_front_frames(64, 40) == -1
    g = lib.fwn_mel_front_frames(1024, 256)
    assert 1 <= g <= 64 and lib.fwn_mel_front_frames(64, 16) >= 1


def test_unit_is_in_the_build_and_clean_of_swizzled_packed_fp32(tmp_path):
    """tools/check_packed_f32.py (tests/test_static_isa.py has the story) over csrc/melfront.hip, built with the Makefile's flags."""
    import re
    import subprocess
    import sys
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import check_packed_f32 as chk
    csrc = os.path.join(root, "tf-flowavenet_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    assert "melfront.hip" in re.search(r"^SRCS\s*=\s*(.*)$", text, re.M).group(1).split()
    assert re.search(r"^melfront\.o:.*stft_lds\.h", text, re.M) and re.search(r"^denoise\.o:.*stft_lds\.h", text, re.M)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(EXTRA)", "").replace("$(ARCH)", arch).split()
    assert "-fno-slp-vectorize" in flags and "-ffp-contract=off" in flags
    out = tmp_path / "melfront.s"
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-c", os.path.join(csrc, "melfront.hip"), "-o", str(out)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ks = list(chk.kernels(str(out)))
    assert sum("peak_abs_kernel" in name for name, _ in ks) == 1 and sum("mel_front_kernel" in name for name, _ in ks) == 2
    flagged = [(name, rep[:2]) for name, body in ks for rep in [chk.check(name, body)] if rep]
    assert not flagged, flagged[:3]
