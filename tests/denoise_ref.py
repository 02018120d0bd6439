"""The spectral denoiser of DESIGN.md 6b restated in NumPy (fp64 by default; ``dtype=np.float32`` runs the same steps in
float32, the yardstick the GPU tests report the kernel's error against).  Not used by the package."""
import numpy as np


def hann(n_fft, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(dtype)


def frame_index(n, n_fft, hop):
    """[F, n_fft] clip indices of the centred reflect-padded frames of a clip of n >= n_fft / 2 + 1 samples."""
    j = np.arange(1 + n // hop)[:, None] * hop + np.arange(n_fft)[None] - n_fft // 2
    j = np.where(j < 0, -j, j)
    return np.where(j >= n, 2 * (n - 1) - j, j)


def frames(x, n_fft, hop):
    """v [F, n_fft]: the windowed frames."""
    x = np.asarray(x)
    return hann(n_fft, x.dtype)[None] * x[frame_index(len(x), n_fft, hop)]


def stft(x, n_fft, hop):
    return np.fft.rfft(frames(x, n_fft, hop), axis=1)


def interior(n, n_fft, hop):
    """(f_min, f_max): the frames whose n_fft samples lie inside a clip of n samples (f_max < f_min: none)."""
    h = n_fft // 2
    return -(-h // hop), (n - h) // hop


def mean_mag(x, n_fft, hop):
    """The bias of rows x [B, N] (or one clip [N]): mean |X[f, k]| over every row's interior frames."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    lo, hi = interior(x.shape[1], n_fft, hop)
    assert hi >= lo, "no interior frame"
    return np.mean([np.abs(stft(row, n_fft, hop))[lo:hi + 1] for row in x], axis=(0, 1))


def envelope(n, n_fft, hop, dtype=np.float64):
    """sum_f w^2 at p = sample + n_fft / 2 for the n samples of a clip."""
    w2 = hann(n_fft, dtype) ** 2
    env = np.zeros(n + 2 * n_fft + hop, dtype=dtype)
    for f in range(1 + n // hop):
        env[f * hop:f * hop + n_fft] += w2
    return env[n_fft // 2:n_fft // 2 + n]


def denoise(x, bias, strength, n_fft, hop):
    """out [N] in x's dtype (float64 unless x is float32)."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        x = x.astype(np.float64)
    n = len(x)
    if n < n_fft // 2 + 1:
        return x.copy()
    dt = x.dtype
    X = stft(x, n_fft, hop)
    if dt == np.float32:
        X = X.astype(np.complex64)
    t = (np.asarray(bias, dtype=dt) * dt.type(strength))[None]
    mag = np.abs(X)
    keep = mag > t
    gain = np.where(keep, 1.0 - t / np.where(keep, mag, 1.0), 0.0).astype(dt)
    y = np.fft.irfft(X * gain, n=n_fft, axis=1).astype(dt)
    w = hann(n_fft, dt)
    acc = np.zeros(n + 2 * n_fft + hop, dtype=dt)
    for f in range(len(y)):                                     # ascending f
        acc[f * hop:f * hop + n_fft] += w * y[f]
    return acc[n_fft // 2:n_fft // 2 + n] / envelope(n, n_fft, hop, dt)


def sample_bound_terms(x, n_fft, hop):
    """(S, env, V): S[n] = sum_f w[p - f hop] ||v_f||_2 over the frames covering sample n, the envelope, and ||v_f||_2 per frame -
    what the per-sample and per-clip error bounds of DESIGN.md 6b are made of."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    V = np.sqrt((frames(x, n_fft, hop) ** 2).sum(axis=1))
    w = hann(n_fft)
    S = np.zeros(n + 2 * n_fft + hop)
    for f in range(len(V)):
        S[f * hop:f * hop + n_fft] += w * V[f]
    return S[n_fft // 2:n_fft // 2 + n], envelope(n, n_fft, hop), V


def pcm16(v):
    """synthesize.write_wav's arithmetic."""
    return (np.clip(np.asarray(v, dtype=np.float64), -1.0, 1.0) * 32767.0).round().astype(np.int16)
