"""TEST INFRASTRUCTURE ONLY - NumPy restatement of the ragged mel front-end (csrc/melfront.hip).

Peak, gain and the padded audio in float32 exactly as the definition has them (they are bit-exact on the device); the mel in
fp64 through ``oracle.mel_np`` on the float32-normalised samples, so that the rounding of the normalisation is not charged to
the mel's bound; and that bound, per element, from the transform's error constant of DESIGN.md 6b.
"""
import numpy as np

from denoise_ref import frame_index
from oracle import mel_np as onp
from tf_flowavenet_amd.hparams import default_hparams

U = 2.0 ** -24
SHAPES = [(1024, 256, 80, 7001), (1024, 256, 80, 513), (64, 16, 8, 33), (64, 16, 8, 1000), (256, 100, 20, 1501)]   # n_fft, hop, n_mels, N


def hp_of(n_fft, hop, n_mels):
    return default_hparams().replace(n_fft=n_fft, hop_size=hop, num_mels=n_mels)


def signal(seed, n, scale=0.1):
    """tests/test_mel.py's noise plus a windowed 440 Hz tone."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    return (scale * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t) * np.hanning(n)).astype(np.float32)


def peak(x):
    """max |x| in float32: +0 for an empty clip, NaN if any sample is."""
    x = np.asarray(x, dtype=np.float32)
    return np.float32(np.abs(x).max()) if len(x) else np.float32(0.0)


def gain(x, pk, rmax):
    """(x / peak) * rmax: two float32 operations - ``_process_utterance``'s ``wav / peak * hparams.rescaling_max``."""
    return (np.asarray(x, dtype=np.float32) / np.float32(pk)) * np.float32(rmax)


def frames_of(n, hop):
    return 1 + n // hop


def padded_audio(xn, hop):
    """The reference's padded, trimmed clip (preprocessing.py:71-84): F hop samples, xn from pad_l = (F hop - N) div 2 on."""
    n = len(xn)
    out = np.zeros(frames_of(n, hop) * hop, dtype=np.float32)
    pad_l = (len(out) - n) // 2
    out[pad_l:pad_l + n] = xn
    return out


def frames64(xn, n_fft, hop):
    """v_f[n] = w[n] xn[j], j = f hop + n - n_fft / 2 reflected, in fp64: [F, n_fft]."""
    xn = np.asarray(xn, dtype=np.float64)
    return xn[frame_index(len(xn), n_fft, hop)] * onp.hann_periodic(n_fft)[None, :]


def db(power, hp):
    mel = 20.0 * np.log10(np.maximum(1e-4, power)) - hp.ref_level_db
    return np.clip((mel - hp.min_level_db) / (-hp.min_level_db), 0.0, 1.0)


def mel64(xn, hp):
    """The definition's own sums in fp64 (the indices above, not ``np.pad``): what the host tests hold against the oracle."""
    X = np.fft.rfft(frames64(xn, hp.n_fft, hp.hop_size), axis=1)
    fb = onp.mel_filterbank(hp.sample_rate, hp.n_fft, hp.num_mels, hp.fmin, hp.fmax)
    return db((X.real ** 2 + X.imag ** 2) @ fb.T, hp)


def front(x, hp, normalize=True):
    """-> (audio float32 [F hop], mel fp64 [F, num_mels], peak float32, xn float32).  A clip that is silent, NaN or shorter
    than n_fft / 2 + 1 samples gives zeros."""
    x = np.asarray(x, dtype=np.float32)
    pk = peak(x)
    f = frames_of(len(x), hp.hop_size)
    if len(x) < hp.n_fft // 2 + 1 or (normalize and not pk > 0.0):
        return np.zeros(f * hp.hop_size, np.float32), np.zeros((f, hp.num_mels)), pk, np.zeros(len(x), np.float32)
    xn = gain(x, pk, hp.rescaling_max) if normalize else x
    return padded_audio(xn, hp.hop_size), onp.melspectrogram(xn.astype(np.float64), hp), pk, xn


def frame_terms(xn, n_fft, hop):
    """The per-frame terms of ``bound`` (and of ``specdist_ref.bound``) for one clip: |X| [F, nb]; e [F, 1], e_f = (16 L + 16) u
    ||v_f||_2, which bounds every bin's error after the transform (DESIGN.md 6b's constant); and dpw [F, nb] = 2 |X| e + e^2 +
    4 u |X|^2, that of the power."""
    v = frames64(xn, n_fft, hop)
    X = np.abs(np.fft.rfft(v, axis=1))
    e = ((16 * np.log2(n_fft) + 16) * U * np.linalg.norm(v, axis=1))[:, None]
    return X, e, 2 * X * e + e ** 2 + 4 * U * X ** 2


def bound(xn, hp, fb):
    """The per-element bound of a float32 evaluation of the mel of the float32 samples ``xn``: [F, num_mels].
    ``frame_terms`` gives e_f and dpw, the error of a bin after the transform and of its power; dP = fb dpw + (nb + 2) u P is that
    of the filter sum; and the log carries it as
    c dP / max(1e-4, P - dP), c = (20 / ln 10) / |min_level_db|, plus 32 u for the log, the affine map and the clip."""
    X, _, dpw = frame_terms(xn, hp.n_fft, hp.hop_size)
    fb = np.asarray(fb, dtype=np.float64)
    P = (X ** 2) @ fb.T
    dP = dpw @ fb.T + (hp.n_fft // 2 + 3) * U * P
    c = (20.0 / np.log(10.0)) / abs(hp.min_level_db)
    return c * dP / np.maximum(1e-4, P - dP) + 32 * U


def mel32(xn, hp, fb):
    """Float32 NumPy: scipy's rfft on float32 frames, float32 filterbank and float32 log - what a correct float32 kernel is like."""
    from scipy.fft import rfft
    X = rfft(frames64(xn, hp.n_fft, hp.hop_size).astype(np.float32), axis=1)
    assert X.dtype == np.complex64
    P = (X.real * X.real + X.imag * X.imag) @ np.asarray(fb, dtype=np.float32).T
    lo, ref = np.float32(hp.min_level_db), np.float32(hp.ref_level_db)
    m = (np.float32(20.0) * np.log10(np.maximum(np.float32(1e-4), P)) - ref - lo) / -lo
    assert m.dtype == np.float32
    return np.clip(m, np.float32(0.0), np.float32(1.0))


def frame_mels32(x, hp, fb):
    """A stand-in for the device's compute step with its locality property: every frame of ``x`` (a clip of its own) on its own,
    so a frame's bits depend on the samples of its support only."""
    from scipy.fft import rfft
    v = frames64(x, hp.n_fft, hp.hop_size).astype(np.float32)
    fb = np.asarray(fb, dtype=np.float32)
    out = np.zeros((len(v), hp.num_mels), dtype=np.float32)
    for f, row in enumerate(v):
        X = rfft(row)
        out[f] = fb @ (X.real * X.real + X.imag * X.imag)
    return out
