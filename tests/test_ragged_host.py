"""Host side of ragged batching (clips of different lengths in one ``reverse`` call): the batch planner of the synthesize
CLI and the C-ABI additions.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import synthesize as S
from tf_flowavenet_amd.hparams import hparams

from conftest import small_hparams


def _t_of(frames, hp):
    align = max(1, (1 << hp.n_block) // int(np.gcd(1 << hp.n_block, hp.hop_size)))
    return (frames + (-frames) % align) * hp.hop_size


def _check_plan(frames, batch, frac, hp):
    groups = S.plan_batches(frames, batch, frac, hp)
    assert sorted(k for g in groups for k in g) == list(range(len(frames)))          # every index exactly once
    for g in groups:
        assert 1 <= len(g) <= batch
        ts = [_t_of(frames[k], hp) for k in g]
        top = max(ts)
        assert len(g) <= S.max_clips_per_call(hp, top)
        if len(g) > 1:
            assert len(g) * top - sum(ts) <= frac * len(g) * top, (g, ts)
    return groups


@pytest.mark.parametrize("batch,frac", [(1, 0.25), (4, 0.0), (8, 0.25), (8, 0.05), (16, 0.6), (3, 1.0)])
def test_plan_batches_covers_every_clip_within_the_batch_and_padding_limits(batch, frac):
    rng = np.random.default_rng(11)
    frames = [int(f) for f in rng.integers(200, 901, size=64)]
    groups = _check_plan(frames, batch, frac, hparams)
    # sorted by length: a group never holds a clip longer than one of a later group
    tops = [max(frames[k] for k in g) for g in groups]
    assert tops == sorted(tops)
    if batch > 1 and frac >= 0.25:
        assert len(groups) < len(frames)          # similar lengths do share calls
    # a model whose hop does not divide by 2^n_block: lengths are compared after the alignment padding
    hp = small_hparams(n_block=5, hop_size=8, upsample_scales=[2, 4])
    _check_plan([1, 2, 3, 4, 5, 9, 13, 16, 17], batch, frac, hp)


def test_plan_batches_groups_equal_lengths_as_the_plain_cli_does():
    frames = [5, 3, 5, 3, 3, 7, 5, 3, 3]
    # no padding allowed: exactly the equal-length grouping, in chunks of `batch`, by length then name
    assert S.plan_batches(frames, 2, 0.0, hparams) == [[1, 3], [4, 7], [8], [0, 2], [6], [5]]
    assert S.plan_batches([4] * 5, 2, 0.25, hparams) == [[0, 1], [2, 3], [4]]
    assert S.plan_batches([4] * 5, 8, 0.25, hparams) == [[0, 1, 2, 3, 4]]
    assert S.plan_batches([], 8, 0.25, hparams) == []


def test_plan_batches_respects_the_per_call_addressing_limit():
    # 10 s clips of the full model: the 2 GiB-per-buffer limit, not --batch, bounds the group
    frames = [862] * 40
    per_call = S.max_clips_per_call(hparams, 862 * hparams.hop_size)
    assert 1 <= per_call < 40
    groups = _check_plan(frames, 64, 0.25, hparams)
    assert max(len(g) for g in groups) == per_call
    with pytest.raises(ValueError, match="exceeds what one call can address"):
        S.plan_batches([S.max_clips_per_call(hparams, 1) // hparams.hop_size + 8], 8, 0.25, hparams)


def test_cli_has_the_ragged_flags(monkeypatch):
    seen = {}
    monkeypatch.setattr(S, "synthesize", lambda args, hp: seen.update(vars(args)))
    S.main(["--ragged", "--max_pad_frac", "0.1", "--batch", "4"])
    assert seen["ragged"] is True and seen["max_pad_frac"] == 0.1 and seen["batch"] == 4
    S.main([])
    assert seen["ragged"] is False and seen["max_pad_frac"] == 0.25


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_ragged_symbols_are_exported_with_their_declared_types_and_the_version_stays(lib):
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {
        "fwn_mask_rows": (C.c_int, [vp, i64, i64, i64, vp, i32, vp]),
        "fwn_ragged_workspace_bytes": (C.c_size_t, [C.POINTER(_lib.ModelDesc), i64, i64]),
        "fwn_model_reverse_ragged": (C.c_int, [C.POINTER(_lib.ModelDesc), i64, i64, vp, vp, vp, vp, C.c_size_t, vp, vp]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert _lib.SIGNATURES[name] == (res, args)
    assert lib.fwn_version() == 322
    # argument validation before any launch
    assert lib.fwn_mask_rows(None, 1, 4, 16, None, 1, None) == -1 and b"fwn_mask_rows" in lib.fwn_last_error()
    assert lib.fwn_mask_rows(1 << 20, 1, 4, 6, 1 << 21, 1, None) == -1 and b"multiples of 4" in lib.fwn_last_error()
    assert lib.fwn_mask_rows(1 << 20, 1, 4, 16, 1 << 21, 0, None) == -1
    m = _lib.ModelDesc()
    assert lib.fwn_ragged_workspace_bytes(C.byref(m), 1, 256) == 0
    assert lib.fwn_model_reverse_ragged(C.byref(m), 1, 256, None, None, None, None, 0, None, None) == -1
