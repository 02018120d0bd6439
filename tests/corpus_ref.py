"""NumPy restatement of the device corpus draw (``fwn_corpus_draw``, include/fwn.h), written from its definition:

  * d = the draw counter (uint64); slot b takes r = Philox4x32-10(counter = (d & 0xffffffff, d >> 32, b, stream_id),
    key = (seed & 0xffffffff, seed >> 32)) - ``philox_ref.philox4x32_10``;
  * u = (r0 * n_utt) >> 32, n = frame_off[u + 1] - frame_off[u];
  * n > F: start = (r1 * (n - F)) >> 32 and F frames; otherwise start = 0 and (n // unit_frames) * unit_frames frames;
  * x [B, F * hop] / c [B, F, num_mels]: the crop, exact zeros past it; len [B] = frames * hop; picks [B, 2] = (u, start).

Python integers for the products (no width to overflow).  A helper module of the tests, not a conftest.
"""
import numpy as np

import philox_ref as P


def mulhi(r, n):
    """The multiply-high map of a 32-bit word r onto [0, n)."""
    return (int(r) * int(n)) >> 32


def pick(r0, r1, frame_off, frames, unit_frames):
    """-> (u, start, clip frames) from the first two words of a slot's Philox output."""
    n_utt = len(frame_off) - 1
    u = mulhi(r0, n_utt)
    n = int(frame_off[u + 1]) - int(frame_off[u])
    if n > frames:
        return u, mulhi(r1, n - frames), frames
    return u, 0, n // unit_frames * unit_frames


def picks(seed, stream_id, counter, batch, frame_off, frames, unit_frames):
    """-> int64 [batch, 3]: (u, start, clip frames) of every slot of draw ``counter``."""
    seed, d = int(seed) % (1 << 64), int(counter) % (1 << 64)
    r = P.philox4x32_10((d & 0xFFFFFFFF, d >> 32, np.arange(batch, dtype=np.uint64), int(stream_id) & 0xFFFFFFFF),
                        (seed & 0xFFFFFFFF, seed >> 32))
    return np.asarray([pick(r[0][b], r[1][b], frame_off, frames, unit_frames) for b in range(batch)], dtype=np.int64).reshape(batch, 3)


def draw(audio, mel, frame_off, hop, frames, unit_frames, batch, seed, stream_id, counter):
    """-> (x float32 [B, F * hop], c float32 [B, F, num_mels], len int32 [B], picks int32 [B, 2]) by NumPy slicing."""
    mel = np.asarray(mel)
    table = picks(seed, stream_id, counter, batch, frame_off, frames, unit_frames)
    x = np.zeros((batch, frames * hop), dtype=np.float32)
    c = np.zeros((batch, frames, mel.shape[1]), dtype=np.float32)
    for b, (u, start, n) in enumerate(table):
        f0 = int(frame_off[u]) + int(start)
        x[b, :n * hop] = audio[f0 * hop:(f0 + n) * hop]
        c[b, :n] = mel[f0:f0 + n]
    return x, c, (table[:, 2] * hop).astype(np.int32), table[:, :2].astype(np.int32)
