"""fp64 NumPy restatement of the sample-rate conversion (DESIGN.md "Sample-rate conversion"; include/fwn.h):

    up = out_rate / gcd, down = in_rate / gcd, q = max(up, down), Hh = zeros * q, n_out(N) = ceil(N up / down)
    h[j] = (up rolloff / q) sinc(rolloff j / q) I0(beta sqrt(1 - (j / Hh)^2)) / I0(beta),   |j| <= Hh
    y[m] = sum_n x[n] h[m down - n up],   |m down - n up| <= Hh,   x = 0 outside [0, N)

Nothing here imports the package: the kernel, the C design function and the Python planning are held to this file.
"""
from __future__ import annotations

from math import gcd

import numpy as np

ZEROS, BETA, ROLLOFF = 32, 10.0, 0.90


def ratio(in_rate, out_rate):
    """(up, down) in lowest terms."""
    g = gcd(int(in_rate), int(out_rate))
    return int(out_rate) // g, int(in_rate) // g


def n_out(n, up, down):
    return -((-int(n) * int(up)) // int(down))


def half_width(up, down, zeros=ZEROS):
    return int(zeros) * max(int(up), int(down))


def taps(up, down, zeros=ZEROS):
    """K: taps per phase."""
    return (2 * half_width(up, down, zeros)) // int(up) + 1


def design(up, down, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """h[-Hh .. Hh] as float64 [2 Hh + 1]; h[j] sits at index j + Hh."""
    q, hh = max(up, down), half_width(up, down, zeros)
    j = np.arange(-hh, hh + 1, dtype=np.float64)
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (j / hh) ** 2))) / np.i0(beta)
    return (up * rolloff / q) * np.sinc(rolloff * j / q) * win


def phase_table(up, down, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """T [up][K] float64, T[r][k] = h[r + k up - Hh], 0 past the support; and the mask of the entries inside it."""
    h, hh, k = design(up, down, zeros, beta, rolloff), half_width(up, down, zeros), taps(up, down, zeros)
    idx = np.arange(up)[:, None] + np.arange(k)[None, :] * up          # j + Hh
    inside = idx <= 2 * hh
    return np.where(inside, h[np.minimum(idx, 2 * hh)], 0.0), inside


def resample_at(x, up, down, m, n_total=None, in_start=0, h=None, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """The direct sum at output positions ``m`` (any int64 values) of a clip of ``n_total`` samples of which ``x`` holds samples
    [in_start, in_start + len(x)) - every sample an output reads must be among them.  -> (y, A, count): float64 values,
    A[m] = sum |x[n] h[.]| and the number of taps inside [0, n_total), per output; 0 for m >= n_out(n_total)."""
    x = np.asarray(x, dtype=np.float64)
    n_total = int(in_start) + len(x) if n_total is None else int(n_total)
    h = design(up, down, zeros, beta, rolloff) if h is None else h
    hh = half_width(up, down, zeros)
    m = np.asarray(m, dtype=np.int64)
    y, a, cnt = np.zeros(len(m)), np.zeros(len(m)), np.zeros(len(m), dtype=np.int64)
    for i, mi in enumerate(m.tolist()):
        if mi < 0 or mi >= n_out(n_total, up, down):
            continue
        lo = max(0, -((hh - mi * down) // up))                        # ceil((m down - Hh) / up)
        hi = min(n_total - 1, (mi * down + hh) // up)
        if lo > hi:
            continue
        assert lo >= in_start and hi < in_start + len(x), "output %d reads samples [%d, %d] outside the span" % (mi, lo, hi)
        n = np.arange(lo, hi + 1, dtype=np.int64)
        terms = x[lo - in_start:hi + 1 - in_start] * h[mi * down - n * up + hh]
        y[i], a[i], cnt[i] = terms.sum(), np.abs(terms).sum(), len(n)
    return y, a, cnt


def resample(x, in_rate, out_rate, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """A whole clip: -> (y, A, count), each of length n_out(len(x))."""
    up, down = ratio(in_rate, out_rate)
    return resample_at(x, up, down, np.arange(n_out(len(x), up, down)), zeros=zeros, beta=beta, rolloff=rolloff)


def bound(a, k):
    """The fp32 dot-product bound of K terms, any order, with or without FMA, plus one rounding of each coefficient."""
    return (k + 2) * 2.0 ** -24 * np.asarray(a)
