"""Device-resident corpus, the part that needs no GPU: the restated draw (tests/corpus_ref.py) at the ends of its map and over
many draws, the flat layout built from a preprocessing directory, the optional checkpoint entry, and the argument checks of
``fwn_corpus_draw``."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_ref as CR  # noqa: E402
import philox_ref as P  # noqa: E402
from test_ragged_train_host import FRAMES, _write  # noqa: E402
from tf_flowavenet_amd import _lib  # noqa: E402

FRAME_COUNTS = (3, 8, 9, 25, 40, 41, 100)
OFF = np.concatenate([[0], np.cumsum(FRAME_COUNTS)]).astype(np.int64)
F = 8


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------ 1. the restated draw
def test_the_multiply_high_map_reaches_both_ends_and_nothing_else():
    for n in (1, 2, 7, 92, 13100, (1 << 31) - 1):
        assert CR.mulhi(0, n) == 0 and CR.mulhi(0xFFFFFFFF, n) == n - 1
    # monotone, onto, and every value takes floor(2^32 / n) or one more of the 2^32 words, counted from the first word of each value
    for n in (3, 7, 92):
        firsts = [-(-(v << 32) // n) for v in range(n + 1)]                   # the smallest r that maps to v
        for v in range(n):
            assert CR.mulhi(firsts[v], n) == v and (firsts[v] == 0 or CR.mulhi(firsts[v] - 1, n) == v - 1)
            assert firsts[v + 1] - firsts[v] in ((1 << 32) // n, (1 << 32) // n + 1)
    # the pick: the utterance from r0, the start from r1, a short utterance whole and floored to the unit
    assert CR.pick(0, 0xFFFFFFFF, OFF, F, 2) == (0, 0, 2)                     # 3 frames -> 2
    assert CR.pick(0, 0xFFFFFFFF, OFF, F, 1) == (0, 0, 3)
    assert CR.pick(0xFFFFFFFF, 0, OFF, F, 2) == (6, 0, F) and CR.pick(0xFFFFFFFF, 0xFFFFFFFF, OFF, F, 2) == (6, 91, F)
    one = (1 << 32) // 7 + 1                                                  # the first word that picks utterance 1: 8 frames = F
    assert CR.pick(one, 0xFFFFFFFF, OFF, F, 2) == (1, 0, 8) and CR.pick(one - 1, 0, OFF, F, 2)[0] == 0


def test_ten_thousand_restated_draws_stay_in_range_and_reach_everything():
    draws, batch = 10000, 2
    seed = (5 << 32) + 75
    d = np.repeat(np.arange(draws, dtype=np.uint64), batch)
    b = np.tile(np.arange(batch, dtype=np.uint64), draws)
    r = P.philox4x32_10((d, 0, b, 1), (seed & 0xFFFFFFFF, seed >> 32))
    table = np.asarray([CR.pick(r[0][k], r[1][k], OFF, F, 2) for k in range(draws * batch)])
    u, start, n = table[:, 0], table[:, 1], table[:, 2]
    frames = np.asarray(FRAME_COUNTS)[u]
    assert u.min() == 0 and u.max() == 6 and set(u) == set(range(7))
    assert (start >= 0).all() and (start + n <= frames).all() and (n >= 2).all() and (n <= F).all() and not (n % 2).any()
    long_ = frames > F
    assert (n[long_] == F).all() and (start[~long_] == 0).all() and (start[long_] < frames[long_] - F).all()
    assert np.array_equal(n[~long_], frames[~long_] // 2 * 2)
    for k, f in enumerate(FRAME_COUNTS):                                      # both extreme starts of every croppable utterance,
        if f > F:                                                             # the shortest one (9 frames: start 0 is both) included
            assert {0, f - F - 1} <= set(start[u == k]) and start[u == k].max() == f - F - 1, f
    # CR.picks is the same table draw by draw, and a larger batch starts with the smaller one
    assert np.array_equal(CR.picks(seed, 1, 17, batch, OFF, F, 2), table[17 * batch:18 * batch])
    assert np.array_equal(CR.picks(seed, 1, 17, 5, OFF, F, 2)[:batch], table[17 * batch:18 * batch])
    assert not np.array_equal(CR.picks(seed, 0, 17, 5, OFF, F, 2), CR.picks(seed, 1, 17, 5, OFF, F, 2))
    assert not np.array_equal(CR.picks(seed, 1, 17 + (1 << 32), 5, OFF, F, 2), CR.picks(seed, 1, 17, 5, OFF, F, 2))


# ------------------------------------------------------------------ 2. the layout
def test_layout_from_a_preprocessing_directory(tmp_path):
    from tf_flowavenet_amd import corpus as DC, train as TL
    hp, path, data = _write(tmp_path, "abcde")
    # utterance c: a mel one frame longer than its audio (41 rows against 40 * hop samples) is cut to the common 40
    mel_c = np.concatenate([data[2][2], np.full((1, hp.num_mels), 99.0, dtype=np.float32)])
    np.save(tmp_path / "mels" / "c-mel.npy", mel_c)
    for ragged in (False, True):
        ds = TL.Dataset(path, hp, seed=3, ragged=ragged)
        lay = DC.CorpusLayout(DC.open_dataset(path, hp, seed=3, ragged=ragged))
        assert lay.meta == ds.train_meta and lay.ragged == ragged             # Dataset's own eligible set, in its order
        names = [m[0][0] for m in lay.meta]
        assert names == (["b", "c", "d", "e"] if ragged else ["c"])
        counts = [FRAMES[k] for k in names]
        assert lay.frame_off.dtype == np.int64 and np.array_equal(lay.frame_off, np.concatenate([[0], np.cumsum(counts)]))
        assert (lay.hop, lay.num_mels, lay.frames, lay.unit_frames, lay.n_utt) == (16, hp.num_mels, 16, 2, len(names))
        assert lay.nbytes == 4 * sum(counts) * (16 + hp.num_mels) + 8 * (len(names) + 1)
        audio, mel = lay.arrays()
        assert audio.dtype == mel.dtype == np.float32 and audio.shape == (sum(counts) * 16,) and mel.shape == (sum(counts), hp.num_mels)
        by_name = {v[0]: v for v in data.values()}
        for u, name in enumerate(names):
            f0, f1 = int(lay.frame_off[u]), int(lay.frame_off[u + 1])
            assert np.array_equal(audio[f0 * 16:f1 * 16], by_name[name][1]) and np.array_equal(mel[f0:f1], by_name[name][2])
        assert not (mel == 99.0).any()
        small = list(lay.chunks(limit=1))                                      # one utterance per piece at the least
        assert [c[0] for c in small] == list(lay.frame_off[:-1])
    # the restated draw over this layout obeys Dataset's rule: b -> 2 frames, e -> 6, d whole, c a 16-frame crop
    x, c, ln, pk = CR.draw(audio, mel, lay.frame_off, 16, 16, 2, 64, 3, 0, 0)
    assert set(pk[:, 0]) == {0, 1, 2, 3}
    for b in range(64):
        want = {0: 32, 1: 256, 2: 256, 3: 96}[int(pk[b, 0])]
        assert ln[b] == want and not x[b, want:].any() and not c[b, want // 16:].any() and x[b, :want].all()
        assert 0 <= pk[b, 1] < (24 if pk[b, 0] == 1 else 1)
    # without lengths nothing may be shorter than the crop: a mel that leaves max_time_steps // hop common frames or fewer
    np.save(tmp_path / "mels" / "c-mel.npy", mel_c[:16])
    with pytest.raises(ValueError, match="common frames"):
        DC.CorpusLayout(TL.Dataset(path, hp, seed=3))
    assert DC.CorpusLayout(TL.Dataset(path, hp, seed=3, ragged=True)).frame_off[2] == 3 + 16


# ------------------------------------------------------------------ 3. the checkpoint entry
def _fake_trainer(fill):
    import torch
    w = {"a/kernel": torch.full((2, 3), float(fill)), "a/bias": torch.full((3,), float(fill) + 1)}
    opt = SimpleNamespace(master_views=lambda: w, m=torch.full((9,), float(fill) + 2), v=torch.full((9,), float(fill) + 3),
                          global_step=int(fill), group=None)
    return SimpleNamespace(opt=opt)


def _fake_corpus(n):
    box = SimpleNamespace(counter=n)
    box.set_counter = lambda v: setattr(box, "counter", int(v))
    return box


def test_checkpoint_entry_is_optional_both_ways(tmp_path):
    from tf_flowavenet_amd import train as TL
    assert TL.DRAW_COUNTER_KEY == "__data/draw_counter"
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir(), new.mkdir()
    TL.save_checkpoint(str(old / "flowavenet_model.ckpt-5.npz"), _fake_trainer(5))
    big = (1 << 40) + 9
    TL.save_checkpoint(str(new / "flowavenet_model.ckpt-7.npz"), _fake_trainer(7), _fake_corpus(big))
    assert TL.DRAW_COUNTER_KEY not in np.load(old / "flowavenet_model.ckpt-5.npz").files
    entry = np.load(new / "flowavenet_model.ckpt-7.npz")[TL.DRAW_COUNTER_KEY]
    assert entry.dtype == np.uint64 and int(entry) == big
    # a checkpoint without the entry loads, with or without a corpus, and leaves the counter alone
    tr, corpus = _fake_trainer(0), _fake_corpus(3)
    assert TL.restore_checkpoint(str(old), tr) == 5 and float(tr.opt.m[0]) == 7.0
    assert TL.restore_checkpoint(str(old), _fake_trainer(0), corpus) == 5 and corpus.counter == 3
    # one with the entry sets it; without a corpus the entry is ignored
    tr = _fake_trainer(0)
    assert TL.restore_checkpoint(str(new), tr, corpus) == 7 and corpus.counter == big and float(tr.opt.master_views()["a/bias"][0]) == 8.0
    assert TL.restore_checkpoint(str(new), _fake_trainer(0)) == 7


def test_the_flag_is_parsed_and_off_by_default(monkeypatch):
    from tf_flowavenet_amd import train as TL
    import torch
    seen = []
    monkeypatch.setattr(TL, "train", lambda log_dir, args, hp, inp: seen.append(args))
    monkeypatch.setattr(torch.cuda, "set_device", lambda k: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    TL.main([])
    TL.main(["--device_corpus", "--ragged", "--accum_steps", "2"])
    assert [a.device_corpus for a in seen] == [False, True] and seen[1].ragged and seen[1].accum_steps == 2


# ------------------------------------------------------------------ 4. the C entry refuses bad arguments
def test_the_entry_refuses_bad_arguments_before_any_launch(lib):
    """FWN_ERR_ARG (-1) with a message naming the entry, on a machine without a GPU: nothing was launched."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fwn.h")).read()
    assert "int fwn_corpus_draw(const float* audio, const float* mel, const int64_t* frame_off, int64_t n_utt, int hop, int num_mels," in header
    assert len(_lib.SIGNATURES["fwn_corpus_draw"][1]) == 17 and lib.fwn_version() == 322       # additive: the version stays
    A = 1 << 20                                                               # never dereferenced
    good = dict(audio=A, mel=2 * A, frame_off=3 * A, n_utt=7, hop=16, num_mels=8, unit_frames=2, B=4, F=8, seed=75, stream_id=0,
                counter=4 * A, x=5 * A, c=6 * A, len=7 * A, picks=8 * A)
    bad = [(dict(audio=None), b"null"), (dict(mel=None), b"null"), (dict(frame_off=None), b"null"), (dict(counter=None), b"null"),
           (dict(x=None), b"null"), (dict(c=None), b"null"), (dict(len=None), b"null"),
           (dict(B=0), b"positive"), (dict(F=0), b"positive"), (dict(n_utt=0), b"positive"), (dict(hop=0), b"positive"),
           (dict(num_mels=0), b"positive"), (dict(unit_frames=0), b"positive"), (dict(B=-1), b"positive"), (dict(hop=-16), b"positive"),
           (dict(B=65536), b"65535"), (dict(n_utt=1 << 31), b"2^31"), (dict(F=1 << 27), b"2^31"),
           (dict(audio=A + 2), b"4-byte"), (dict(x=5 * A + 1), b"4-byte"), (dict(picks=8 * A + 2), b"4-byte"),
           (dict(frame_off=3 * A + 4), b"8-byte"), (dict(counter=4 * A + 4), b"8-byte")]
    for change, word in bad:
        a = dict(good, **change)
        assert lib.fwn_corpus_draw(*a.values(), None) == -1, change
        msg = lib.fwn_last_error()
        assert b"fwn_corpus_draw" in msg and word in msg, (change, msg)
