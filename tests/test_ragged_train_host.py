"""Host side of the ragged training step (no GPU): what ``train.py --ragged`` feeds the step, the one validation path of the
lengths, and the argument checks of the new C entry points."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import small_hparams
from tf_flowavenet_amd import _lib, model as M, train as TL, training as TR

# hop 16, 2^n_block = 32: the unit of a ragged clip is 32 samples = 2 frames; max_time_steps = 16 frames
HP = dict(n_block=5, max_time_steps=256, batch_size=6, test_size=100)
FRAMES = {"a": 1, "b": 3, "c": 40, "d": 16, "e": 7}


def _write(tmp_path, names):
    hp = small_hparams(**HP)
    for sub in ("audios", "mels"):
        (tmp_path / sub).mkdir(exist_ok=True)
    lines, data = [], {}
    for k, name in enumerate(names):
        f = FRAMES[name]
        audio = (np.arange(f * hp.hop_size, dtype=np.float32) + 1.0) * 1e-4 + k           # every sample names its utterance and position
        mel = (np.arange(f, dtype=np.float32)[:, None] + 1.0) * 1e-2 + k + np.zeros((1, hp.num_mels), dtype=np.float32)
        np.save(tmp_path / "audios" / ("%s-audio.npy" % name), audio)
        np.save(tmp_path / "mels" / ("%s-mel.npy" % name), mel)
        lines.append("%s-audio.npy|%s-mel.npy|%d|0|text" % (name, name, len(audio)))
        data[k] = (name, audio, mel)
    (tmp_path / "train.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    return hp, str(tmp_path / "train.txt"), data


def test_ragged_dataset_keeps_short_utterances_whole_and_crops_long_ones(tmp_path):
    hp, path, data = _write(tmp_path, "abcde")
    ds = TL.Dataset(path, hp, seed=3, ragged=True)
    kept = sorted(m[0][0] for m in ds.train_meta)
    assert kept == ["b", "c", "d", "e"]                                       # the 1-frame utterance is below the unit: dropped
    seen = set()
    for draw in range(8):
        mels, audios, lengths = ds.next_train() if draw % 2 == 0 else ds.next_test()
        assert mels.shape == (6, 16, hp.num_mels) and audios.shape == (6, 256) and mels.dtype == audios.dtype == np.float32
        assert lengths.shape == (6,) and lengths.dtype == np.int32
        for k in range(6):
            who = int(round(float(audios[k, 0])))                             # the utterance's index rides its samples
            name, audio, mel = data[who]
            seen.add(name)
            n = int(lengths[k])
            assert n % 32 == 0 and 32 <= n <= 256
            want = {"b": 32, "c": 256, "d": 256, "e": 96}[name]             # 3 -> 2 frames, 40 -> a 16-frame crop, 16 whole, 7 -> 6 frames
            assert n == want, (name, n)
            if name == "c":                                                   # cropped at a random start
                start = int(np.argmin(np.abs(audio - audios[k, 0])))
                assert start % hp.hop_size == 0 and 0 <= start // hp.hop_size < 40 - 16
            else:                                                             # whole, from its first sample
                start = 0
            assert np.array_equal(audios[k, :n], audio[start:start + n])
            assert np.array_equal(mels[k, :n // hp.hop_size], mel[start // hp.hop_size:(start + n) // hp.hop_size])
            assert not audios[k, n:].any() and not mels[k, n // hp.hop_size:].any()       # the lengths match the arrays
    assert seen == {"b", "c", "d", "e"}
    # the data-dependent init batch: full-length crops only, no lengths
    mels, audios = ds.next_full()
    assert mels.shape == (6, 16, hp.num_mels) and all(int(round(float(a[0]))) == 2 for a in audios)


def test_dataset_without_the_flag_is_unchanged(tmp_path):
    hp, path, data = _write(tmp_path, "abcde")
    ds = TL.Dataset(path, hp, seed=3)
    assert [m[0][0] for m in ds.train_meta] == ["c"]                          # strictly longer than max_time_steps only
    out = ds.next_train()
    assert len(out) == 2 and out[0].shape == (6, 16, hp.num_mels) and out[1].shape == (6, 256)
    # the crops are those of the same generator calls as ever: one draw for the picks, one start per clip (dataset.py:73-76)
    rng = np.random.RandomState(3)
    rng.randint(0, 1, size=6)
    for k in range(6):
        start = rng.randint(0, 40 - 16)
        assert np.array_equal(out[1][k], data[2][1][start * 16:start * 16 + 256])
        assert np.array_equal(out[0][k], data[2][2][start:start + 16])
    assert len(ds.next_test()) == 2


def test_dataset_error_messages(tmp_path):
    hp, path, _ = _write(tmp_path, "abe")
    with pytest.raises(ValueError, match="no utterance longer than max_time_steps=256"):
        TL.Dataset(path, hp)
    ds = TL.Dataset(path, hp, ragged=True)                                    # short prompts only: they train
    assert len(ds.next_train()) == 3
    with pytest.raises(ValueError, match="init=True takes no lengths"):
        ds.next_full()
    hp, path, _ = _write(tmp_path, "a")
    with pytest.raises(ValueError, match="at least lcm"):
        TL.Dataset(path, hp, ragged=True)


BAD = ([64, 64], [64, 64, 64, 64], [64, 24, 64], [64, 80, 64], [64, 0, 64], [64, 8, 64], [64, -16, 64], [64, 32.5, 64], 64)


def test_length_validation_is_shared_with_the_model(monkeypatch):
    """``GradEngine.check_lengths`` and ``FloWaveNet._check_lengths`` are one function, ``model.check_lengths``: same values,
    same messages, and a change to it reaches both."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    hp = small_hparams()
    eng = TR.GradEngine(hp)
    fake = SimpleNamespace(hop=hp.hop_size, _hparams=hp)
    assert eng.check_lengths(np.asarray([64, 16, 48]), 3, 64) == M.FloWaveNet._check_lengths(fake, [64, 16, 48], 3, 64) == [64, 16, 48]
    for bad in BAD:
        msgs = []
        for fn in (lambda: eng.check_lengths(bad, 3, 64), lambda: M.FloWaveNet._check_lengths(fake, bad, 3, 64)):
            with pytest.raises(ValueError) as e:
                fn()
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
    calls = []
    monkeypatch.setattr(M, "check_lengths", lambda *a: calls.append(a) or [1, 2, 3])
    assert eng.check_lengths([64, 16, 48], 3, 64) == [1, 2, 3]
    assert M.FloWaveNet._check_lengths(fake, [64, 16, 48], 3, 64) == [1, 2, 3]
    assert calls == [([64, 16, 48], 3, 64, hp.hop_size, hp.n_block)] * 2
    with pytest.raises(ValueError, match="gate_fp8"):
        TR.GradEngine(hp.replace(gate_fp8=True)).check_lengths([64, 16, 48], 3, 64)


def test_new_entry_points_validate_their_arguments():
    """No launch happens for bad arguments: error code + message (CPU-only check)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    td = _lib.TrainDesc()
    assert lib.fwn_train_ragged_workspace_bytes(C.byref(td), 2, 128) == 0
    cb = _lib.BLOCK_DONE_FN(lambda user, blk: 0)
    assert lib.fwn_train_loss_and_grads_ragged(C.byref(td), 2, 128, 1 << 20, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20, None, cb, None, None) == -1
    assert b"null lengths" in lib.fwn_last_error()
    assert lib.fwn_train_loss_and_grads_ragged(C.byref(td), 2, 128, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, None, cb, None, None) == -1
    assert b"null descriptor" in lib.fwn_last_error()
    g = _lib.GemmDesc()
    g.W, g.Y, g.nseg, g.M, g.N, g.Ti, g.ldw, g.ldy, g.nsplit, g.out_f32 = 1 << 20, 1 << 21, 1, 64, 64, 32, 64, 64, 1, 1
    g.seg[0].x, g.seg[0].rows, g.seg[0].ld, g.seg[0].k = 1 << 22, 64, 64, 64
    g.row_len, g.len_spr, g.accumulate = 1 << 23, 2, 1
    assert lib.fwn_gemm(C.byref(g), None) == -1 and b"refused together with accumulate" in lib.fwn_last_error()
    g.accumulate, g.len_spr = 0, 0
    assert lib.fwn_gemm(C.byref(g), None) == -1 and b"row_len" in lib.fwn_last_error()
    g.len_spr, g.Ti = 2, 48                                                   # M is no multiple of Ti
    assert lib.fwn_gemm(C.byref(g), None) == -1 and b"row_len" in lib.fwn_last_error()
    assert lib.fwn_coupling_bwd_ragged(None, None, None, None, 2, 4, 1, None, 2, None, 8, None, None, None, 0, None) == -1
    assert b"fwn_coupling_bwd_ragged" in lib.fwn_last_error()
    assert lib.fwn_flow_small_grads_ragged(*([None] * 6), 2, 4, 1, None, 2, *([None] * 7)) == -1
    assert b"fwn_flow_small_grads_ragged" in lib.fwn_last_error()
    assert C.sizeof(_lib.GemmDesc) == 400 and _lib.GemmDesc.row_len.offset == 384
