"""CPU tests of the sample-rate conversion: the fp64 restatement (tests/resample_ref.py) against scipy and against the filter
properties the definition promises, ``fwn_resample_design`` / ``fwn_resample_taps`` against the restatement's table, the
C entry's refusals (no launch), ``ResampleStream``'s planning on the restatement, and ``preprocessing.load_wav``'s readers."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import resample_ref as R
from tf_flowavenet_amd import _lib

PAIRS = [(48000, 22050), (44100, 22050), (22050, 8000), (16000, 22050), (22050, 48000), (24000, 22050), (22050, 44100),
         (11025, 8000), (8000, 22050), (96000, 8000)]
LENGTHS = [1, 7, 1000, 4097]
CHECKED = [(48000, 22050), (22050, 8000), (16000, 22050)]      # the pairs whose filter figures DESIGN.md states


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- the restatement against scipy ----

@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_restatement_equals_scipy_resample_poly(in_rate, out_rate):
    from scipy.signal import resample_poly
    up, down = R.ratio(in_rate, out_rate)
    h = R.design(up, down)
    rng = np.random.default_rng(in_rate + out_rate)
    for n in LENGTHS:
        x = rng.uniform(-1.0, 1.0, n)
        y, _, _ = R.resample(x, in_rate, out_rate)
        want = resample_poly(x, up, down, window=h / up, padtype="constant")       # scipy multiplies a given filter by up
        assert len(y) == len(want) == R.n_out(n, up, down)
        err = float(np.abs(y - want).max())
        print("%d -> %d, n = %d: max |restatement - scipy| = %.2e" % (in_rate, out_rate, n, err))
        assert err <= 1e-12


# ---- filter properties of the restatement ----

def _response_db(h, up, q):
    """|H| in dB relative to the ideal pass-band gain `up`, on a dense grid: -> (f, dB), f in units of the narrower Nyquist
    (pi / q on h's grid), from 0 to h's own Nyquist (f = q) in steps of q / 2^20."""
    mag = np.abs(np.fft.rfft(h, 1 << 21)) / up                 # zero phase is not needed for the magnitude
    return np.arange(len(mag)) * (q / float(1 << 20)), 20.0 * np.log10(np.maximum(mag, 1e-300))


@pytest.mark.parametrize("in_rate,out_rate", CHECKED)
def test_restatement_filter_ripple_and_stop_band(in_rate, out_rate):
    up, down = R.ratio(in_rate, out_rate)
    q, h = max(up, down), R.design(up, down)
    f, db = _response_db(h, up, q)
    ripple, stop = db[f <= 0.80], db[f >= 1.00]
    six = f[np.argmax(db <= -6.0206)]                          # where the response first falls to one half
    print("%d -> %d: ripple %+.2e .. %+.2e dB to 0.80, -6 dB at %.4f, stop band %.1f dB from 1.00"
          % (in_rate, out_rate, ripple.min(), ripple.max(), six, stop.max()))
    assert np.abs(ripple).max() <= 2e-4
    assert stop.max() <= -99.0
    assert abs(six - 0.90) <= 0.002


def test_restatement_tones_48000_to_22050():
    n = 24000
    t_in, t_out = np.arange(n) / 48000.0, np.arange(R.n_out(n, 147, 320)) / 22050.0
    edge = 32 * 320 // 147 + 2                      # outputs whose support reaches past the clip: the zero padding shows there
    y, _, _ = R.resample(np.sin(2 * np.pi * 1000.0 * t_in), 48000, 22050)
    err = float(np.abs(y - np.sin(2 * np.pi * 1000.0 * t_out))[edge:-edge].max())
    z, _, _ = R.resample(np.sin(2 * np.pi * 12200.0 * t_in), 48000, 22050)
    leak = 20.0 * np.log10(float(np.abs(z[edge:-edge]).max()))
    print("1 kHz tone: max error %.2e; 12.2 kHz tone: %.1f dB" % (err, leak))
    assert err <= 1e-5
    assert leak <= -100.0


# ---- fwn_resample_design / fwn_resample_taps against the restatement's table ----

@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_design_matches_restatement_within_one_ulp(lib, in_rate, out_rate):
    from tf_flowavenet_amd.resample import design_table, ratio
    up, down = R.ratio(in_rate, out_rate)
    assert ratio(in_rate, out_rate) == (up, down)
    k = R.taps(up, down)
    assert lib.fwn_resample_taps(up, down, R.ZEROS) == k
    got = design_table(up, down)
    assert got.shape == (up, k) and got.dtype == np.float32
    want, inside = R.phase_table(up, down)
    assert np.all(got[~inside] == 0.0)                         # the zeros of the layout are exact zeros
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32))
    assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), float(np.abs(got - want).max())
    print("%d/%d: K = %d, %d bytes, %d of %d entries differ from the rounded fp64 table"
          % (up, down, k, got.nbytes, int((got != w32).sum()), got.size))


def test_design_other_parameters(lib):
    from tf_flowavenet_amd.resample import design_table
    for zeros, beta, rolloff in ((1, 0.0, 1.0), (8, 5.0, 0.5), (64, 14.0, 0.95)):
        got = design_table(3, 2, zeros, beta, rolloff)
        want, inside = R.phase_table(3, 2, zeros, beta, rolloff)
        assert got.shape == want.shape == (3, R.taps(3, 2, zeros))
        assert np.all(got[~inside] == 0.0)
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want.astype(np.float32))))


# ---- refusals: -1, the function's name in the message, nothing launched (this runs where there is no GPU) ----

def test_design_and_taps_refusals(lib):
    buf = np.zeros(64 * 200, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for args in ((4, 2, 32, 10.0, 0.9), (320, 147 * 2, 32, 10.0, 0.9),      # gcd != 1
                 (3, 2, 0, 10.0, 0.9), (3, 2, 65, 10.0, 0.9),               # zeros outside 1..64
                 (3, 2, 8, 10.0, 0.0), (3, 2, 8, 10.0, 1.01), (3, 2, 8, 10.0, -0.5), (3, 2, 8, 10.0, float("nan")),
                 (3, 2, 8, -1.0, 0.9), (3, 2, 8, float("nan"), 0.9),
                 (0, 2, 8, 10.0, 0.9), (3, -1, 8, 10.0, 0.9)):
        assert lib.fwn_resample_design(*args, p) == -1, args
        assert b"fwn_resample_design" in lib.fwn_last_error(), args
    assert np.all(buf == 0.0)
    assert lib.fwn_resample_design(3, 2, 8, 10.0, 0.9, None) == -1 and b"fwn_resample_design" in lib.fwn_last_error()
    for args in ((4, 2, 32), (3, 2, 0), (3, 2, 65), (0, 1, 32)):
        assert lib.fwn_resample_taps(*args) == -1, args
        assert b"fwn_resample_taps" in lib.fwn_last_error(), args
    with pytest.raises(_lib.FwnError, match="fwn_resample"):
        from tf_flowavenet_amd.resample import design_table
        design_table(4, 2)


def test_resample_refusals_before_any_launch(lib):
    """Every refusal returns before the launch: the pointers below are not device memory, and no device is needed."""
    P = 1 << 20                                    # an aligned non-null "pointer" that is never dereferenced

    def call(x=P, pcm=0, B=1, xs=1000, start=0, n_in=1000, lens=None, n=1000, tab=P, up=147, down=320, zeros=32, y=P, ys=460,
             m0=0, n_out=460):
        rc = lib.fwn_resample(x, pcm, B, xs, start, n_in, lens, n, tab, up, down, zeros, y, ys, m0, n_out, None)
        if rc != 0:
            assert b"fwn_resample" in lib.fwn_last_error()
        return rc

    assert call(x=None) == -1 and call(tab=None) == -1 and call(y=None) == -1
    assert call(up=294, down=640) == -1 and b"lowest terms" in lib.fwn_last_error()
    assert call(zeros=0) == -1 and call(zeros=65) == -1
    assert call(pcm=2) == -1
    assert call(x=P + 2) == -1 and call(y=P + 2) == -1 and call(tab=P + 1) == -1 and call(lens=P + 4) == -1
    assert call(x=P + 1, pcm=1) == -1
    assert call(B=0) == -1 and call(B=65536) == -1
    assert call(n=-1) == -1 and call(start=-1) == -1 and call(n_in=-1) == -1 and call(m0=-1) == -1 and call(n_out=0) == -1
    assert call(xs=999) == -1 and call(ys=459) == -1
    assert call(up=1, down=100, n_out=10, ys=10) == -1 and b"fit" in lib.fwn_last_error()       # 31 903 floats of LDS per tile
    # the provided span must hold every requested output's support inside [0, N)
    assert call(start=1) == -1 and b"provided span" in lib.fwn_last_error()                 # output 0 reads sample 0
    assert call(n_in=999, xs=999) == -1 and b"provided span" in lib.fwn_last_error()        # output 459 reads sample 999
    hh, up, down = 32 * 320, 147, 320
    m0 = 300
    lo = -((hh - m0 * down) // up)                  # first sample output 300 reads
    assert lo > 0
    assert call(start=lo + 1, n_in=1000 - lo - 1, xs=1000, m0=m0, n_out=160, ys=160) == -1
    hi = (349 * down + hh) // up                    # last sample output 349 reads
    assert hi < 999
    assert call(start=lo, n_in=hi - lo, xs=1000, m0=m0, n_out=50, ys=50) == -1


# ---- ResampleStream's planning, with the restatement as the compute step ----

@pytest.mark.parametrize("in_rate,out_rate", [(48000, 22050), (22050, 48000), (96000, 8000)])
def test_stream_on_the_restatement_equals_one_call(in_rate, out_rate):
    from tf_flowavenet_amd.resample import ResampleStream, out_length
    up, down = R.ratio(in_rate, out_rate)
    h, k = R.design(up, down), R.taps(up, down)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, 50000)
    whole, _, _ = R.resample(x, in_rate, out_rate)
    assert len(whole) == out_length(len(x), up, down)

    def compute(hist, in_start, n_total, m0, n_out):
        return R.resample_at(hist, up, down, np.arange(m0, m0 + n_out), n_total=n_total, in_start=in_start, h=h)[0]

    for chunk in (1, 4096, 7777):
        if chunk == 1 and (in_rate, out_rate) != (48000, 22050):
            continue                                # one pair at one sample per push is enough (50 000 pushes)
        s = ResampleStream(up, down, R.ZEROS, compute)
        parts, worst = [], 0
        for a in range(0, len(x), chunk):
            out = s.push(x[a:a + chunk])
            if out is not None:
                parts.append(out)
            worst = max(worst, s.retained)
            assert s.retained <= k                  # only what the filter's support still needs
        tail = s.finish()
        if tail is not None:
            parts.append(tail)
        got = np.concatenate(parts)
        assert got.shape == whole.shape and np.array_equal(got, whole), (chunk, len(got), len(whole))
        assert len(parts) > 1 and worst > 0
        with pytest.raises(RuntimeError):
            s.push(x[:1])


def test_stream_of_a_short_clip_and_of_nothing():
    from tf_flowavenet_amd.resample import ResampleStream
    up, down = R.ratio(22050, 8000)
    for n in (0, 1, 5):
        x = np.linspace(0.1, 0.9, n)

        def compute(hist, in_start, n_total, m0, n_out):
            return R.resample_at(hist, up, down, np.arange(m0, m0 + n_out), n_total=n_total, in_start=in_start)[0]

        s = ResampleStream(up, down, R.ZEROS, compute)
        assert s.push(x) is None                    # every support reaches past the clip's end: nothing is computable yet
        tail = s.finish()
        if n == 0:
            assert tail is None
        else:
            assert np.array_equal(tail, R.resample(x, 22050, 8000)[0])


# ---- load_wav ----

def _write(path, rate, width, frames):
    """frames: int array [n] or [n, channels] of PCM values in the width's own range."""
    frames = np.asarray(frames)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if frames.ndim == 1 else frames.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        flat = frames.reshape(-1)
        if width == 1:
            raw = flat.astype(np.uint8).tobytes()
        elif width == 3:
            v = flat.astype(np.int64) & 0xFFFFFF
            raw = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=1).astype(np.uint8).tobytes()
        else:
            raw = flat.astype({2: "<i2", 4: "<i4"}[width]).tobytes()
        w.writeframes(raw)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_load_wav_reads_every_pcm_width_and_stereo(tmp_path, width):
    from tf_flowavenet_amd.preprocessing import load_wav
    bits = 8 * width
    lo, hi = (0, 255) if width == 1 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    rng = np.random.default_rng(width)
    mono = np.concatenate([[lo, hi, 0 if width > 1 else 128, lo + 1], rng.integers(lo, hi + 1, 500)])
    stereo = np.stack([mono, mono[::-1]], axis=1)

    def floats(v):
        v = np.asarray(v, dtype=np.float64)
        return (((v - 128.0) / 128.0) if width == 1 else v / float(1 << (bits - 1))).astype(np.float32)

    _write(tmp_path / "m.wav", 22050, width, mono)
    got = load_wav(str(tmp_path / "m.wav"), 22050)
    assert got.dtype == np.float32 and np.array_equal(got, floats(mono))
    assert got.min() == -1.0 and (got.max() < 1.0 or width == 4)       # (2^31 - 1) / 2^31 rounds to 1.0 in float32
    _write(tmp_path / "s.wav", 22050, width, stereo)
    got = load_wav(str(tmp_path / "s.wav"), 22050)
    assert got.dtype == np.float32 and np.array_equal(got, floats(stereo).mean(axis=1))


def test_load_wav_equals_read_wav_and_read_wav_still_refuses(tmp_path):
    from tf_flowavenet_amd.preprocessing import load_wav, read_wav
    pcm = np.random.default_rng(0).integers(-32768, 32768, (300, 2))
    _write(tmp_path / "a.wav", 22050, 2, pcm)
    assert np.array_equal(load_wav(str(tmp_path / "a.wav"), 22050), read_wav(str(tmp_path / "a.wav"), 22050))
    with pytest.raises(ValueError, match="resample first"):
        read_wav(str(tmp_path / "a.wav"), 16000)
    _write(tmp_path / "b.wav", 22050, 3, pcm[:, 0] * 256)
    with pytest.raises(ValueError, match="16-bit"):
        read_wav(str(tmp_path / "b.wav"), 22050)
