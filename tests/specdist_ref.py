"""TEST INFRASTRUCTURE ONLY - NumPy restatement of the spectral distances (csrc/specdist.hip).

``dist`` is the definition in fp64 on the float32 samples; ``bound`` what a float32 evaluation of it may differ by, derived from
``mel_front_ref``'s per-frame terms (the transform's error constant of DESIGN.md 6b); ``dist32`` a float32 NumPy evaluation, to
see how much of the bound a correct float32 kernel needs; ``NumpyMetric`` a stand-in for ``metrics.SpectralDistance`` with the
same interface, for the CLI's host tests.
"""
import numpy as np

import mel_front_ref as MR

U = MR.U
FLOOR = 1e-4
SHAPES = [(1024, 256, 80), (512, 96, 80), (32, 16, 4), (2048, 512, 16), (4096, 2048, 8)]      # n_fft, hop, n_mels
FRAMES = 8                                                     # what fwn_spectral_distance_frames returns


def lengths_of(n_fft, hop, frames=FRAMES):
    """The shortest clip there is; one workgroup's frames exactly (F = frames) and one sample short of it (F = frames - 1); the
    first frame of the second workgroup, minus one sample, exact and plus one; three workgroups plus one frame."""
    return [n_fft // 2 + 1, (frames - 1) * hop - 1, (frames - 1) * hop, frames * hop - 1, frames * hop, frames * hop + 1, 3 * frames * hop]


def pair(seed, n, scale=0.1):
    """Noise plus a tone (``mel_front_ref.signal``) against a perturbed copy: a gain, and noise a tenth as strong."""
    x = MR.signal(seed, n, scale)
    rng = np.random.default_rng(seed + 1000)
    y = (np.float32(0.9) * x + np.float32(0.1 * scale) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return x, y


def power64(x, n_fft, hop):
    """|X_f[k]|^2 in fp64: [F, nb]."""
    X = np.fft.rfft(MR.frames64(x, n_fft, hop), axis=1)
    return X.real ** 2 + X.imag ** 2


def mel64(x, hp, fb):
    """``fwn_mel_front``'s mel with ``peak_dev = NULL`` in fp64, over the filterbank the device reads."""
    return MR.db(power64(x, hp.n_fft, hp.hop_size) @ np.asarray(fb, dtype=np.float64).T, hp)


def _ldb(p, floor):
    return 10.0 * np.log10(np.maximum(floor, p))


def terms(px, py, floor):
    """(lsd_db, sc) from two power arrays [F, nb], in the arrays' own precision for the terms and fp64 for the sums."""
    d = _ldb(px, floor) - _ldb(py, floor)
    lsd = np.sqrt((d * d).astype(np.float64).mean(axis=1)).mean()
    m = np.sqrt(px) - np.sqrt(py)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.sqrt((m * m).astype(np.float64).sum()) / np.sqrt(px.astype(np.float64).sum())
    return float(lsd), float(sc)


def dist(x, y, n_fft, hop, hp=None, fb=None, floor=FLOOR):
    """-> (mel_l1, lsd_db, sc, frames) in fp64.  ``hp`` and ``fb`` (the model's, at n_fft / hop) give mel_l1; without them NaN.
    A pair shorter than n_fft / 2 + 1 samples: NaN, NaN, NaN, 0."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert x.shape == y.shape and x.ndim == 1
    if len(x) < n_fft // 2 + 1:
        return float("nan"), float("nan"), float("nan"), 0
    px, py = power64(x, n_fft, hop), power64(y, n_fft, hop)
    lsd, sc = terms(px, py, floor)
    mel = float("nan")
    if fb is not None:
        assert (hp.n_fft, hp.hop_size) == (n_fft, hop)
        fb = np.asarray(fb, dtype=np.float64)
        mel = float(np.abs(MR.db(px @ fb.T, hp) - MR.db(py @ fb.T, hp)).mean())
    return mel, lsd, sc, MR.frames_of(len(x), hop)


def dist32(x, y, n_fft, hop, hp=None, fb=None, floor=FLOOR):
    """The same in float32 NumPy (scipy's float32 rfft, float32 terms, fp64 sums): what a correct float32 kernel is like."""
    from scipy.fft import rfft
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if len(x) < n_fft // 2 + 1:
        return float("nan"), float("nan"), float("nan"), 0
    p = []
    for c in (x, y):
        X = rfft(MR.frames64(c, n_fft, hop).astype(np.float32), axis=1)
        assert X.dtype == np.complex64
        p.append(X.real * X.real + X.imag * X.imag)
    lsd, sc = terms(p[0], p[1], np.float32(floor))
    mel = float("nan")
    if fb is not None:
        mel = float(np.abs(MR.mel32(x, hp, fb) - MR.mel32(y, hp, fb)).astype(np.float64).mean())
    return mel, lsd, sc, MR.frames_of(len(x), hop)


def bound(x, y, n_fft, hop, hp=None, fb=None, floor=FLOOR):
    """-> (b_mel, b_lsd, b_sc): what a float32 evaluation of ``dist`` may differ from it by.

    mel_l1  | |a' - b'| - |a - b| | <= |a' - a| + |b' - b| per (f, m): the mean over (f, m) of the two clips' own
            ``mel_front_ref.bound``s, plus u for the float32 difference of two values in [0, 1].
    lsd_db  a bin's level 10 log10 max(floor, P) is off by d = (10 / ln 10) dpw / max(floor, P - dpw) + 4 u |10 log10 max(floor, P)|
            (the power's error through the logarithm's slope, and the float32 log10, product and difference); a frame's lsd_f is
            the 2-norm of the level differences over sqrt(nb), and | ||a'|| - ||a|| | <= ||a' - a||: sqrt(mean_k (dx_k + dy_k)^2),
            averaged over the frames.
    sc      a magnitude is off by e_f (the transform) + 3 u |X| (dpw's own 4 u |X|^2 through the root, and the root): over all
            (f, k), E = sqrt(nb sum_f e_f^2) + 3 u ||X||.  The numerator n = || |X| - |Y| || moves by at most Ex + Ey + 2 u n, the
            denominator D = ||X|| by Ex + u D, and the quotient by (dn + sc dD) / (D - dD)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    nb = n_fft // 2 + 1
    X, ex, dpx = MR.frame_terms(x, n_fft, hop)
    Y, ey, dpy = MR.frame_terms(y, n_fft, hop)
    b_mel = float("nan")
    if fb is not None:
        b_mel = float((MR.bound(x, hp, fb) + MR.bound(y, hp, fb)).mean() + U)

    def level_err(A, dp):
        P = A ** 2
        return (10.0 / np.log(10.0)) * dp / np.maximum(floor, P - dp) + 4 * U * np.abs(_ldb(P, floor))
    d = level_err(X, dpx) + level_err(Y, dpy)
    b_lsd = float(np.sqrt((d ** 2).mean(axis=1)).mean())
    nx, ny = np.sqrt((X ** 2).sum()), np.sqrt((Y ** 2).sum())
    Ex = np.sqrt(nb * (ex ** 2).sum()) + 3 * U * nx
    Ey = np.sqrt(nb * (ey ** 2).sum()) + 3 * U * ny
    n = np.sqrt(((X - Y) ** 2).sum())
    dn, dD = Ex + Ey + 2 * U * n, Ex + U * nx
    b_sc = float((dn + (n / nx) * dD) / (nx - dD))
    return b_mel, b_lsd, b_sc


def shares(got, ref, bd):
    """|got - ref| / bound of the three measures (0 where both are 0)."""
    out = []
    for g, r, b in zip(got[:3], ref[:3], bd):
        if np.isnan(r) and np.isnan(g):
            out.append(0.0)
        else:
            out.append(abs(g - r) / b if b > 0 else (0.0 if g == r else float("inf")))
    return out


class NumpyMetric:
    """``metrics.SpectralDistance``'s interface over ``dist32`` (or ``dist``): host arrays or CPU tensors in, a dict of float64
    ``[B]`` NumPy arrays out.  ``calls`` records the shapes and lengths of every call."""

    def __init__(self, hp, resolutions=None, floor=FLOOR, fn=dist32):
        from tf_flowavenet_amd.metrics import combine
        from tf_flowavenet_amd.preprocessing import mel_filterbank
        self._hp, self._fb, self._fn, self._combine = hp, mel_filterbank(hp), fn, combine
        self.own = (hp.n_fft, hp.hop_size)
        self.resolutions = [self.own] if resolutions is None else [tuple(r) for r in resolutions]
        self.floor = floor
        self.calls = []

    def _block(self, x, y, lens, n_fft, hop, mel):
        rows = [self._fn(a[:n], b[:n], n_fft, hop, self._hp if mel else None, self._fb if mel else None, self.floor)
                for a, b, n in zip(x, y, lens)]
        return np.array(rows, dtype=np.float64)

    def dist(self, ref, test, lengths=None):
        x = np.atleast_2d(np.asarray(ref, dtype=np.float32))
        y = np.atleast_2d(np.asarray(test, dtype=np.float32))
        assert x.shape == y.shape
        lens = [x.shape[1]] * len(x) if lengths is None else [int(n) for n in lengths]
        self.calls.append((x.shape, list(lens)))
        own = self._block(x, y, lens, self.own[0], self.own[1], True)
        per = [own if r == self.own else self._block(x, y, lens, r[0], r[1], False) for r in self.resolutions]
        return self._combine(per, own, self.resolutions)


# ---- every refusal of fwn_spectral_distance, with plausible (never dereferenced) addresses: all come before any launch ----
Q = 1 << 24
REFUSALS = [(dict(n_fft=100), b"power of two"), (dict(n_fft=16), b"power of two"), (dict(n_fft=8192), b"power of two"),
            (dict(hop=0), b"hop"), (dict(hop=33), b"hop"),
            (dict(x=None), b"null"), (dict(y=None), b"null"), (dict(out=None), b"null"),
            (dict(x=Q + 2), b"alignment"), (dict(y=2 * Q + 1), b"alignment"), (dict(fb=10 * Q + 2), b"alignment"),
            (dict(bands=11 * Q + 2), b"alignment"), (dict(len_dev=Q + 4), b"alignment"), (dict(out=3 * Q + 4), b"alignment"),
            (dict(ws=4 * Q + 4), b"alignment"),
            (dict(B=0), b"1..65535"), (dict(B=65536), b"1..65535"),
            (dict(len_host=0), b"2^40"), (dict(len_host=(1 << 40) + 1, xs=1 << 41, ys=1 << 41), b"2^40"),
            (dict(xs=999), b"stride"), (dict(ys=999), b"stride"), (dict(xs=(1 << 44) + 1), b"stride"), (dict(ys=(1 << 44) + 1), b"stride"),
            (dict(n_mels=0), b"n_mels"), (dict(n_mels=1025), b"n_mels"),
            (dict(fb=None), b"bands without fb"),
            (dict(lo=0.0), b"min_level_db"), (dict(lo=5.0), b"min_level_db"), (dict(lo=float("nan")), b"min_level_db"),
            (dict(floor=0.0), b"floor"), (dict(floor=-1e-4), b"floor"), (dict(floor=float("inf")), b"floor"),
            (dict(floor=float("nan")), b"floor"),
            (dict(ws=None), b"workspace"), (dict(wsb=511), b"workspace"), (dict(wsb=0), b"workspace"),
            (dict(out=Q + 4000), b"overlaps"), (dict(out=2 * Q + 7992), b"overlaps"), (dict(out=Q - 8), b"overlaps"),
            (dict(ws=Q + 7992), b"overlaps"), (dict(ws=2 * Q - 504), b"overlaps"), (dict(ws=3 * Q + 56), b"overlaps"),
            (dict(len_host=1 << 40, xs=1 << 40, ys=1 << 40, hop=1, B=1), b"workgroups")]


def refusal_call(lib, **kw):
    """B = 2 rows of 1000 samples at n_fft 64, hop 16 (63 frames: 8 workgroups, 512 bytes of workspace), one argument changed."""
    a = dict(x=Q, xs=1000, y=2 * Q, ys=1000, B=2, len_dev=None, len_host=1000, fb=10 * Q, bands=11 * Q, n_fft=64, hop=16, n_mels=8,
             ref=20.0, lo=-100.0, floor=1e-4, out=3 * Q, ws=4 * Q, wsb=512)
    a.update(kw)
    return lib.fwn_spectral_distance(a["x"], a["xs"], a["y"], a["ys"], a["B"], a["len_dev"], a["len_host"], a["fb"], a["bands"],
                                     a["n_fft"], a["hop"], a["n_mels"], a["ref"], a["lo"], a["floor"], a["out"], a["ws"], a["wsb"], None)
