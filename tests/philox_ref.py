"""fp64 NumPy restatement of the device latent stream (``fwn_latent_normal``, include/fwn.h), written from its definition:

  * Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds;
  * key (seed & 0xffffffff, seed >> 32), counter (q, 0, clip_id, 0) with q = i // 4 for sample i of the clip;
  * the output words r0..r3 give samples 4q..4q+3: for the pairs (r0, r1) and (r2, r3), u1 = ((r >> 8) + 1) 2^-24,
    u2 = (r' >> 8) 2^-24, rad = sqrt(-2 ln u1), samples rad cos(2 pi u2) and rad sin(2 pi u2), times temp.

Everything is ``uint64`` arithmetic masked to 32 bits and float64 from the bits on.  A helper module of the tests, not a conftest.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    c = [np.broadcast_to(v, np.broadcast(*c).shape).copy() for v in c]
    k0, k1 = (int(key[0]) & 0xFFFFFFFF), (int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]              # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def latent_normal(seed, clip_id, n, temp=1.0):
    """The first n samples of clip ``clip_id`` under ``seed`` (taken mod 2^64): float64 [n]."""
    seed = int(seed) % (1 << 64)
    nq = (int(n) + 3) // 4
    r = philox4x32_10((np.arange(nq, dtype=np.uint64), 0, int(clip_id) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, seed >> 32))
    out = np.empty((nq, 4), dtype=np.float64)
    for pair in range(2):
        u1 = ((r[2 * pair] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (r[2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pair] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:int(n)] * float(temp)


def latent_batch(seed, clip_ids, t, temp=1.0, lengths=None):
    """float64 [B, t]: row b is clip ``clip_ids[b]``; with ``lengths`` the samples at i >= lengths[b] are 0."""
    z = np.stack([latent_normal(seed, k, t, temp) for k in clip_ids])
    if lengths is not None:
        for b, n in enumerate(lengths):
            z[b, int(n):] = 0.0
    return z


def pcm16(x):
    """``write_wav``'s arithmetic: clip to [-1, 1] in float64, times 32767, round half to even, int16."""
    return (np.clip(np.asarray(x).astype(np.float64), -1.0, 1.0) * 32767.0).round().astype("<i2")
