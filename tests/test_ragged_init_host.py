"""Host side of the ragged ActNorm init (no GPU): the batch ``train.py --ragged`` feeds it, the flags, and the argument checks of
the new C entry points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ragged_train_host import _write
from tf_flowavenet_amd import _lib, train as TL


def test_next_init_on_a_corpus_of_short_utterances_only(tmp_path):
    hp, path, data = _write(tmp_path, "abe")
    ds = TL.Dataset(path, hp, seed=3, ragged=True)
    assert not ds.has_full()
    out = ds.next_init()
    assert len(out) == 3
    mels, audios, lengths = out
    assert mels.shape == (6, 16, hp.num_mels) and audios.shape == (6, 256) and lengths.shape == (6,) and lengths.dtype == np.int32
    for k in range(6):
        name, audio, mel = data[int(round(float(audios[k, 0])))]
        n = int(lengths[k])
        assert n == {"b": 32, "e": 96}[name]                                  # 3 -> 2 frames, 7 -> 6 frames: whole, floored to the unit
        assert np.array_equal(audios[k, :n], audio[:n]) and np.array_equal(mels[k, :n // hp.hop_size], mel[:n // hp.hop_size])
        assert not audios[k, n:].any() and not mels[k, n // hp.hop_size:].any()
    # drawn as next_train draws: the same generator calls
    a, b = TL.Dataset(path, hp, seed=3, ragged=True).next_init(), TL.Dataset(path, hp, seed=3, ragged=True).next_train()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError, match="init=True takes no lengths"):       # next_full stays as it is
        ds.next_full()


def test_next_init_without_ragged_is_next_trains_pair(tmp_path):
    hp, path, _ = _write(tmp_path, "abcde")
    out = TL.Dataset(path, hp, seed=3).next_init()
    assert len(out) == 2 and out[0].shape == (6, 16, hp.num_mels) and out[1].shape == (6, 256)
    want = TL.Dataset(path, hp, seed=3).next_train()
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    ds = TL.Dataset(path, hp, seed=3, ragged=True)
    assert ds.has_full() and len(ds.next_init()) == 3


def test_cli_flags(monkeypatch):
    seen = {}
    monkeypatch.setattr(TL, "train", lambda log_dir, args, hp, inp: seen.update(vars(args)))
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    TL.main(["--ragged", "--ragged_init"])
    assert seen["ragged"] is True and seen["ragged_init"] is True
    TL.main(["--ragged"])
    assert seen["ragged"] is True and seen["ragged_init"] is False


def test_new_entry_points_validate_their_arguments():
    """No launch happens for bad arguments: error code + message (CPU-only check)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    m = _lib.ModelDesc()
    assert lib.fwn_ragged_init_workspace_bytes(C.byref(m), 2, 128) == 0
    assert lib.fwn_model_forward_init_ragged(C.byref(m), 2, 128, 1 << 20, 1 << 20, None, 1 << 20, 1 << 20, 1 << 20, None, None, None, None) == -1
    assert b"null lengths" in lib.fwn_last_error()
    assert lib.fwn_model_forward_init_ragged(C.byref(m), 2, 128, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, None, None, None, None) == -1
    assert b"model desc" in lib.fwn_last_error()
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(3, 70001, 1) == 51 * 4 * 8        # about 4096 elements of a plane per chunk
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(2, 3000, 64) == 64 * 4 * 64 * 8   # 64 chunks at most
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(6, 37, 1) == 4 * 8
    assert lib.fwn_actnorm_moments_ragged_scratch_bytes(2, 4, 3) == 0 and lib.fwn_actnorm_moments_ragged_scratch_bytes(70000, 4, 2) == 0
    big = 1 << 20
    assert lib.fwn_actnorm_moments_ragged(big, big, 2, 4, 2, None, 4, big, big, 1 << 20, None) == -1
    assert b"fwn_actnorm_moments_ragged" in lib.fwn_last_error()
    assert lib.fwn_actnorm_moments_ragged(big, big, 2, 4, 3, big, 4, big, big, 1 << 20, None) == -1 and b"power of two" in lib.fwn_last_error()
    assert lib.fwn_actnorm_moments_ragged(big, big, 2, 4, 2, big, 4, big, big, 8, None) == -1 and b"scratch" in lib.fwn_last_error()
