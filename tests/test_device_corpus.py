"""Device-resident corpus on the GPU (-m gpu): ``fwn_corpus_draw`` bit for bit against the NumPy restatement of its stream
(tests/corpus_ref.py) and NumPy slicing, its counter, a captured draw, corpora past 2^31 samples; ``Trainer`` on a drawn batch
against the same batch through host arrays and host lengths; ``train.py --device_corpus`` resumed against run straight through.

Every comparison is exact: the draw copies and zero-fills, and the training step sees the same bits either way."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corpus_ref as CR  # noqa: E402
from conftest import small_hparams  # noqa: E402
from tf_flowavenet_amd import _lib  # noqa: E402
from tf_flowavenet_amd import weights as W  # noqa: E402
from tf_flowavenet_amd.training import DeviceLengths, Trainer  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = dict(n_block=3, n_flow=2, n_layer=2, hop_size=16, upsample_scales=[4, 4], num_mels=16)      # tests/test_accum.py's
FRAME_COUNTS = (3, 8, 9, 25, 40, 41, 100)
F = 8
GUARD = 64
SENTINEL = 12345.678
SEEDS = (75, (5 << 32) + 75)


def _flat(frame_counts, hop, num_mels, seed=0):
    """A corpus of seeded noise without a zero in it: (audio [frames * hop], mel [frames, num_mels], frame_off)."""
    rng = np.random.default_rng(seed)
    total = int(sum(frame_counts))
    audio = rng.standard_normal(total * hop).astype(np.float32)
    mel = rng.standard_normal((total, num_mels)).astype(np.float32)
    audio[audio == 0], mel[mel == 0] = 1.0, 1.0
    return audio, mel, np.concatenate([[0], np.cumsum(frame_counts)]).astype(np.int64)


def _guarded(n, off, dtype=torch.float32, inner=float("nan"), guard=SENTINEL):
    """A buffer of n elements ``off`` elements past a 16-byte boundary, filled with ``inner``, ``guard`` all around it."""
    buf = torch.full((GUARD + off + n + GUARD,), guard, dtype=dtype, device="cuda")
    buf[GUARD + off:GUARD + off + n] = inner
    return buf


class _Corpus:
    """The flat arrays on the device, ``off`` elements past a 16-byte boundary, and a draw counter."""

    def __init__(self, audio, mel, frame_off, hop, off=0):
        self.hop, self.num_mels, self.off = hop, mel.shape[1], off
        self.host = (audio, mel, frame_off)
        self.audio = _guarded(audio.size, off)
        self.audio[GUARD + off:GUARD + off + audio.size] = torch.from_numpy(audio).cuda()
        self.mel = _guarded(mel.size, off)
        self.mel[GUARD + off:GUARD + off + mel.size] = torch.from_numpy(mel.reshape(-1)).cuda()
        self.frame_off = torch.from_numpy(frame_off).cuda()
        self.counter = torch.zeros(1, dtype=torch.int64, device="cuda")

    def buffers(self, b, frames=F):
        return (_guarded(b * frames * self.hop, self.off), _guarded(b * frames * self.num_mels, self.off),
                _guarded(b, self.off, torch.int32, -1, -77), _guarded(2 * b, self.off, torch.int32, -1, -77))

    def draw(self, bufs, b, unit, seed, stream_id, frames=F, picks=True):
        lib = _lib.load()
        at = lambda t, size: t.data_ptr() + size * (GUARD + self.off)
        x, c, ln, pk = bufs
        rc = lib.fwn_corpus_draw(at(self.audio, 4), at(self.mel, 4), self.frame_off.data_ptr(), len(self.host[2]) - 1, self.hop,
                                 self.num_mels, unit, b, frames, seed, stream_id, self.counter.data_ptr(), at(x, 4), at(c, 4), at(ln, 4),
                                 at(pk, 4) if picks else None, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "fwn_corpus_draw")

    def check(self, bufs, b, unit, seed, stream_id, counter, frames=F, picks=True, what=()):
        """The buffers against the restated draw ``counter``, by bit pattern; the guards untouched."""
        audio, mel, frame_off = self.host
        want = CR.draw(audio, mel, frame_off, self.hop, frames, unit, b, seed, stream_id, counter)
        sizes = (b * frames * self.hop, b * frames * self.num_mels, b, 2 * b)
        for k, (buf, n, ref) in enumerate(zip(bufs, sizes, want)):
            host = buf.cpu().numpy()
            lo = GUARD + self.off
            guard = np.concatenate([host[:lo], host[lo + n:]])
            assert (guard == (np.float32(SENTINEL) if k < 2 else -77)).all(), ("guard", k) + what
            got = host[lo:lo + n]
            if k == 3 and not picks:
                assert (got == -1).all(), what
                continue
            ref = ref.reshape(-1)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (("x", "c", "len", "picks")[k],) + what
        return want


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("hop,num_mels", [(256, 80), (96, 80), (6, 5)])
def test_draws_equal_the_restatement_and_numpy_slicing_bit_for_bit(hop, num_mels):
    """(6, 5): rows that are no multiple of 16 bytes, the dword path; ``off`` = 1 puts every base one element past a 16-byte
    boundary, the dword path for the other two.  Five consecutive draws per setting, every output pre-filled with NaN (-1
    for the integers): all of x, c and len is written by every call, zeros past each clip exactly."""
    host = _flat(FRAME_COUNTS, hop, num_mels)
    seen_u, short, cropped = set(), 0, 0
    for off in (0, 1):
        corpus = _Corpus(*host, hop, off)
        for unit in (1, 2):
            for b in (1, 3, 8):
                for seed in SEEDS:
                    for stream_id in (0, 1):
                        first = 3 if b == 3 else 0
                        corpus.counter.fill_(first)
                        for k in range(5):
                            bufs = corpus.buffers(b)
                            picks = not (b == 3 and k == 4)                   # the optional table left out once
                            corpus.draw(bufs, b, unit, seed, stream_id, picks=picks)
                            want = corpus.check(bufs, b, unit, seed, stream_id, first + k, picks=picks,
                                                what=(off, unit, b, seed, stream_id, k))
                            seen_u |= set(int(u) for u in want[3][:, 0])
                            short += int((want[2] < F * hop).sum())
                            cropped += int((want[3][:, 1] > 0).sum())
                        assert int(corpus.counter.item()) == first + 5
    assert seen_u == set(range(7)) and short > 0 and cropped > 0              # the cases were all there


def test_only_longer_utterances_give_full_length_clips():
    """The non-ragged rule: the eligible set holds only utterances of more than F frames, and then every length is F hop."""
    hop, num_mels = 96, 80
    corpus = _Corpus(*_flat([n for n in FRAME_COUNTS if n > F], hop, num_mels, seed=1), hop)
    for k in range(5):
        bufs = corpus.buffers(8)
        corpus.draw(bufs, 8, 2, SEEDS[0], 0)
        want = corpus.check(bufs, 8, 2, SEEDS[0], 0, k)
        assert (want[2] == F * hop).all()
        assert not torch.isnan(bufs[0]).any() and not (bufs[0][GUARD:GUARD + 8 * F * hop] == 0).any()


def test_the_counter_advances_by_one_per_call_from_a_value_above_two_to_the_32():
    hop, num_mels = 6, 5
    corpus = _Corpus(*_flat(FRAME_COUNTS, hop, num_mels), hop)
    start = (3 << 32) + 0xFFFFFFFE                                            # the low word wraps into the high one on the way
    corpus.counter.fill_(start)
    tables = []
    for k in range(4):
        bufs = corpus.buffers(8)
        corpus.draw(bufs, 8, 1, SEEDS[1], 1)
        assert int(corpus.counter.item()) == start + k + 1
        tables.append(corpus.check(bufs, 8, 1, SEEDS[1], 1, start + k)[3])
    assert not np.array_equal(tables[0], CR.draw(*corpus.host, hop, F, 1, 8, SEEDS[1], 1, start & 0xFFFFFFFF)[3])   # the high word counts
    assert len({t.tobytes() for t in tables}) == 4


def test_a_captured_draw_replayed_four_times_gives_the_eager_sequence():
    hop, num_mels = 96, 80
    corpus = _Corpus(*_flat(FRAME_COUNTS, hop, num_mels), hop)
    bufs = corpus.buffers(8)
    corpus.draw(bufs, 8, 2, SEEDS[0], 0)                                      # both kernels have run once before the capture
    corpus.counter.fill_(11)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        corpus.draw(bufs, 8, 2, SEEDS[0], 0)
    torch.cuda.synchronize()
    assert int(corpus.counter.item()) == 11                                   # capturing draws nothing
    kept = []
    for k in range(4):
        graph.replay()
        kept.append(tuple(t.clone() for t in bufs))
    torch.cuda.synchronize()
    assert int(corpus.counter.item()) == 15
    for k in range(4):
        corpus.check(kept[k], 8, 2, SEEDS[0], 0, 11 + k, what=("replay", k))
    # ... which is what four eager calls give
    corpus.counter.fill_(11)
    for k in range(4):
        eager = corpus.buffers(8)
        corpus.draw(eager, 8, 2, SEEDS[0], 0)
        for a, b in zip(eager, kept[k]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_offsets_past_two_to_the_31_samples():
    """Two utterances whose samples lie past 2^31 (and whose bytes past 2^33) in ``torch.empty`` arrays: only their own rows are
    written, every draw picks one of them, and the batch holds exactly their data."""
    if torch.cuda.mem_get_info()[0] < (16 << 30):
        pytest.skip("needs 16 GB of free device memory")
    hop, num_mels = 256, 4
    first = (1 << 31) // hop + 3                                              # the first frame past sample 2^31
    frame_off = np.asarray([first, first + 20, first + 26], dtype=np.int64)
    total = int(frame_off[-1])
    rng = np.random.default_rng(2)
    own_audio = rng.standard_normal(26 * hop).astype(np.float32)
    own_mel = rng.standard_normal((26, num_mels)).astype(np.float32)
    audio = mel = None
    try:
        audio = torch.empty(total * hop, dtype=torch.float32, device="cuda")
        mel = torch.empty(total, num_mels, dtype=torch.float32, device="cuda")
        audio[first * hop:] = torch.from_numpy(own_audio).cuda()
        mel[first:] = torch.from_numpy(own_mel).cuda()
        table = torch.from_numpy(frame_off).cuda()
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        lib = _lib.load()
        seen = set()
        for k in range(3):
            x, c = _guarded(8 * F * hop, 0), _guarded(8 * F * num_mels, 0)
            ln, pk = _guarded(8, 0, torch.int32, -1, -77), _guarded(16, 0, torch.int32, -1, -77)
            at = lambda t, size: t.data_ptr() + size * GUARD
            _lib.check(lib.fwn_corpus_draw(audio.data_ptr(), mel.data_ptr(), table.data_ptr(), 2, hop, num_mels, 2, 8, F, SEEDS[1], 0,
                                           counter.data_ptr(), at(x, 4), at(c, 4), at(ln, 4), at(pk, 4),
                                           torch.cuda.current_stream().cuda_stream), "fwn_corpus_draw")
            # the restatement over the two utterances alone: the same table moved to frame 0
            want = CR.draw(own_audio, own_mel, frame_off - first, hop, F, 2, 8, SEEDS[1], 0, k)
            for buf, ref in zip((x, c, ln, pk), want):
                host = buf.cpu().numpy()
                ref = ref.reshape(-1)
                assert np.array_equal(host[GUARD:GUARD + ref.size].view(np.uint32), ref.view(np.uint32)), k
                assert (host[:GUARD] == host[-1]).all() and (host[GUARD + ref.size:] == host[-1]).all()
            seen |= set(int(u) for u in want[3][:, 0])
        assert seen == {0, 1}
    finally:
        del audio, mel
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 2. DeviceCorpus and the training step
def _corpus_dir(root, hp, frame_counts, seed=0):
    """A preprocessing output of seeded noise: ``train.txt``, ``audios/``, ``mels/`` -> the path of train.txt."""
    rng = np.random.default_rng(seed)
    for sub in ("audios", "mels"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    lines = []
    for k, f in enumerate(frame_counts):
        audio = (0.3 * rng.standard_normal(f * hp.hop_size)).astype(np.float32)
        mel = rng.standard_normal((f, hp.num_mels)).astype(np.float32)
        np.save(os.path.join(root, "audios", "u%d-audio.npy" % k), audio)
        np.save(os.path.join(root, "mels", "u%d-mel.npy" % k), mel)
        lines.append("u%d-audio.npy|u%d-mel.npy|%d|0|text" % (k, k, len(audio)))
    path = os.path.join(root, "train.txt")
    with open(path, "wt", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")
    return path


TRAIN_FRAMES = (3, 16, 17, 40, 9, 25, 5, 33)              # F = 16: four short ones (one of exactly F frames), four to crop


def _train_hp():
    return small_hparams(max_time_steps=256, batch_size=4, test_size=100, **CFG)


def test_device_corpus_draws_what_the_restatement_draws_from_the_layout(tmp_path):
    from tf_flowavenet_amd import corpus as DC, train as TL
    hp = _train_hp()
    path = _corpus_dir(str(tmp_path), hp, TRAIN_FRAMES)
    with pytest.raises(MemoryError, match=r"takes \d+ bytes"):
        DC.DeviceCorpus(path, hp, seed=3, ragged=True, max_bytes=1000)
    for ragged in (True, False):
        corpus = DC.DeviceCorpus(path, hp, seed=3, rank=1, ragged=ragged)
        lay = corpus.layout
        assert lay.meta == TL.Dataset(path, hp, seed=3, ragged=ragged).train_meta and lay.n_utt == (8 if ragged else 4)
        audio, mel = lay.arrays()
        corpus.set_counter((1 << 33) + 1)
        assert corpus.counter == (1 << 33) + 1
        ptrs = None
        for k in range(3):
            x, c, lengths = corpus.draw(4)
            want = CR.draw(audio, mel, lay.frame_off, 16, 16, 1, 4, 3, 1, (1 << 33) + 1 + k)
            assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
            assert np.array_equal(corpus.picks.cpu().numpy(), want[3])
            if ragged:
                assert isinstance(lengths, DeviceLengths) and np.array_equal(lengths.tensor.cpu().numpy(), want[2])
            else:
                assert lengths is None and (want[2] == 256).all()
            now = (x.data_ptr(), c.data_ptr(), None if lengths is None else lengths.tensor.data_ptr())
            assert ptrs in (None, now)                                        # the same tensors every call
            ptrs = now
        assert corpus.counter == (1 << 33) + 4


def _params(hp):
    return W.synthetic_params(hp, 11)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "recorded"])
def test_step_and_accumulate_on_a_drawn_batch_equal_the_host_path_bit_for_bit(tmp_path, graph):
    """Two trainers from the same masters: one takes the drawn device tensors and ``DeviceLengths``, the other the same batch
    as NumPy arrays and host lengths.  Three updates of accumulate + step: with ``graph`` the recordings go from the eager
    warm-up through the capture to a replay."""
    from tf_flowavenet_amd import corpus as DC, train as TL
    hp = _train_hp()
    path = _corpus_dir(str(tmp_path), hp, TRAIN_FRAMES)
    ds = TL.Dataset(path, hp, seed=3, ragged=True)
    corpus = DC.DeviceCorpus(ds, hp, seed=3)
    mels, audios = ds.next_full()
    dev_tr, host_tr = Trainer(hp, _params(hp), graph=graph), Trainer(hp, _params(hp), graph=graph)
    for tr in (dev_tr, host_tr):
        tr.ddi(audios, mels)
    short = 0
    for update in range(3):
        for kind in ("accumulate", "step"):
            x, c, lengths = corpus.draw(4)
            hx, hc, hl = x.cpu().numpy(), c.cpu().numpy(), lengths.tensor.cpu().numpy()
            short += int((hl < 256).sum())
            got = getattr(dev_tr, kind)(x, c, lengths=lengths)
            want = getattr(host_tr, kind)(hx, hc, lengths=hl)
            torch.cuda.synchronize()
            what = (update, kind)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), what
            assert all(torch.equal(a, b) for a, b in zip(dev_tr.per_clip, host_tr.per_clip)), what
            for name in ("g", "w", "m", "v"):
                assert torch.equal(getattr(dev_tr.opt, name), getattr(host_tr.opt, name)), what + (name,)
        assert dev_tr.opt.global_step == host_tr.opt.global_step == update + 1 and dev_tr.pending == 0
    assert short > 0 and bool(dev_tr.opt.g.any())
    assert bool(dev_tr._recorded_acc) == graph


# ------------------------------------------------------------------ 3. train.py
def _args(base, **kw):
    a = dict(base_dir=base, restore=True, summary_interval=4, checkpoint_interval=100, eval_interval=1000, train_steps=4, seed=3,
             ragged=True, accum_steps=2, device_corpus=True)
    a.update(kw)
    return SimpleNamespace(**a)


def test_a_resumed_run_continues_the_data_stream(tmp_path):
    """4 updates straight through against 2 updates, a restore and 2 more: masters, Adam slots and the draw counter are
    bit-identical.  Update 1 is the init step on the host Dataset's batch; updates 2 .. 4 take draws (0, 1), (2, 3), (4, 5)."""
    from tf_flowavenet_amd import corpus as DC, train as TL
    hp = _train_hp()
    base = str(tmp_path)
    path = _corpus_dir(base, hp, TRAIN_FRAMES)
    straight = TL.train(os.path.join(base, "logs_a"), _args(base), hp, "train.txt")
    TL.train(os.path.join(base, "logs_b"), _args(base, train_steps=2), hp, "train.txt")
    resumed = TL.train(os.path.join(base, "logs_b"), _args(base), hp, "train.txt")
    assert sorted(os.listdir(resumed)) == ["flowavenet_model.ckpt-2.npz", "flowavenet_model.ckpt-4.npz"]
    a, b = (dict(np.load(os.path.join(d, "flowavenet_model.ckpt-4.npz"))) for d in (straight, resumed))
    assert int(np.load(os.path.join(resumed, "flowavenet_model.ckpt-2.npz"))[TL.DRAW_COUNTER_KEY]) == 2
    assert int(a[TL.DRAW_COUNTER_KEY]) == int(b[TL.DRAW_COUNTER_KEY]) == 6 and int(a["__opt/global_step"]) == 4
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    # the summary of update 4 reads the lengths of its two draws from the device
    lay = DC.CorpusLayout(TL.Dataset(path, hp, seed=3, ragged=True))
    lens = np.concatenate([CR.picks(3, 0, d, 4, lay.frame_off, 16, 1)[:, 2] * 16 for d in (4, 5)])
    for logs in ("logs_a", "logs_b"):
        recs = [json.loads(line) for line in open(os.path.join(base, logs, "train", "summary.jsonl"))]
        assert [r["step"] for r in recs] == [4] and recs[0]["mean_clip_length"] == float(np.mean(lens.astype(np.int32)))


def test_without_the_flag_the_batches_are_the_datasets(tmp_path, monkeypatch):
    """No ``--device_corpus``: the first three batches are those of a ``Dataset`` built alongside (the init batch, then
    ``next_train``), as NumPy arrays with host lengths - and ``fwn_corpus_draw`` is never called."""
    from tf_flowavenet_amd import corpus as DC, train as TL
    hp = _train_hp()
    base = str(tmp_path)
    path = _corpus_dir(base, hp, TRAIN_FRAMES)
    calls = []

    def spy(self, x, c, lengths=None, _real=Trainer.step):
        calls.append((x, c, lengths))
        return _real(self, x, c, lengths)

    monkeypatch.setattr(Trainer, "step", spy)
    monkeypatch.setattr(DC.DeviceCorpus, "draw", lambda self, b: pytest.fail("a draw without the flag"))
    args = _args(base, device_corpus=False, accum_steps=1, train_steps=3, restore=False)
    del args.device_corpus                                                    # a caller that predates the flag
    TL.train(os.path.join(base, "logs"), args, hp, "train.txt")
    shadow = TL.Dataset(path, hp, seed=3, ragged=True)
    mels, audios = shadow.next_full()
    want = [(audios, mels, None)] + [(a, m, l) for m, a, l in (shadow.next_train() for _ in range(2))]
    assert len(calls) == 3
    for (x, c, lengths), (wx, wc, wl) in zip(calls, want):
        assert isinstance(x, np.ndarray) and np.array_equal(x, wx) and np.array_equal(c, wc)
        assert (lengths is None) == (wl is None) and (wl is None or np.array_equal(lengths, wl))
