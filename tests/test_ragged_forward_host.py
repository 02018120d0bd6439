"""Host side of the ragged forward pass (per-clip log_p / logdet for clips of different lengths in one ``forward`` call): the
C-ABI additions and the grouping and cropping of the ``score`` CLI.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import score as SC
from tf_flowavenet_amd import synthesize as S
from tf_flowavenet_amd.hparams import hparams

from conftest import small_hparams


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_ragged_forward_symbols_are_exported_with_their_declared_types_and_the_version_stays(lib):
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {
        "fwn_ragged_forward_workspace_bytes": (C.c_size_t, [C.POINTER(_lib.ModelDesc), i64, i64]),
        "fwn_model_forward_ragged": (C.c_int, [C.POINTER(_lib.ModelDesc), i64, i64, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]),
        "fwn_fill_neg_shift": (C.c_int, [vp, i64, i64, C.c_int, vp, vp, i32, vp]),
        "fwn_ragged_logdet_slots": (C.c_int, [i64]),
        "fwn_ragged_logdet_rows": (C.c_int, [vp, i64, i64, C.c_int, vp, vp, vp, i32, vp, vp]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert _lib.SIGNATURES[name] == (res, args)
    assert lib.fwn_version() == 322
    # argument validation before any launch
    assert lib.fwn_fill_neg_shift(None, 1, 4, 4, None, None, 1, None) == -1 and b"fwn_fill_neg_shift" in lib.fwn_last_error()
    assert lib.fwn_fill_neg_shift(1 << 20, 1, 4, 3, 1 << 21, 1 << 22, 1, None) == -1 and b"power of two" in lib.fwn_last_error()
    assert lib.fwn_fill_neg_shift((1 << 20) + 2, 1, 4, 4, 1 << 21, 1 << 22, 1, None) == -1 and b"aligned" in lib.fwn_last_error()
    assert lib.fwn_fill_neg_shift(1 << 20, 1, 4, 4, 1 << 21, 1 << 22, 0, None) == -1
    assert lib.fwn_ragged_logdet_rows(None, 1, 4, 4, None, None, None, 1, None, None) == -1
    assert lib.fwn_ragged_logdet_rows(1 << 20, 1, 4, 6, 1 << 21, None, 1 << 22, 8, 1 << 23, None) == -1
    assert lib.fwn_ragged_logdet_rows(1 << 20, 1, 4, 4, 1 << 21, None, 1 << 22, 8, (1 << 23) + 4, None) == -1
    # chunk sums plus the ActNorm slot: at least two slots per clip, never more workgroups than a few thousand over all clips
    assert lib.fwn_ragged_logdet_slots(0) == 0
    for b in (1, 4, 64, 2047, 2048, 32767):
        n = lib.fwn_ragged_logdet_slots(b)
        assert 2 <= n <= 33 and (n - 1) * b <= max(2048, b)
    m = _lib.ModelDesc()
    assert lib.fwn_ragged_forward_workspace_bytes(C.byref(m), 1, 256) == 0
    assert lib.fwn_model_forward_ragged(C.byref(m), 1, 256, None, None, None, None, 0, None, None, None) == -1


def test_ragged_forward_workspace_exceeds_the_plain_one_and_leaves_the_others_alone(lib):
    """A descriptor whose pointers are never followed: the sizes come from the geometry alone."""
    hp = small_hparams(n_block=3)
    nfl = hp.n_block * hp.n_flow
    flows = (_lib.FlowDesc * nfl)()
    for i in range(hp.n_block):
        for j in range(hp.n_flow):
            d = flows[i * hp.n_flow + j]
            d.Ch, d.L, d.cin, d.npt = 1 << i, hp.n_layer, (hp.num_mels // 2) * (2 << i), 1
            d.kcpad, d.kfpad = 64, 64
            for f in ("Wfront", "bfront", "Wskip", "bskip", "Wfinal", "bfinal", "Wzero", "bzero", "ezero", "an"):
                setattr(d, f, 1 << 20)
            for l in range(hp.n_layer):
                d.Wd[l] = d.Wc[l] = d.bgate[l] = d.Wres[l] = d.bres[l] = 1 << 20
    m = _lib.ModelDesc()
    m.n_block, m.n_flow, m.n_layer, m.num_mels, m.n_up = hp.n_block, hp.n_flow, hp.n_layer, hp.num_mels, len(hp.upsample_scales)
    for k, s in enumerate(hp.upsample_scales):
        m.up_scale[k], m.up_w[k] = s, 1 << 20
    m.flows = flows
    for b, t in ((1, 64), (4, 256), (3, 4096)):
        plain = lib.fwn_workspace_bytes(C.byref(m), b, t)
        ragged = lib.fwn_ragged_workspace_bytes(C.byref(m), b, t)
        fwd = lib.fwn_ragged_forward_workspace_bytes(C.byref(m), b, t)
        assert plain > 0, lib.fwn_last_error()
        assert fwd > ragged > plain
        # on top of the inverse's: one flow's Z (B T fp32) and the fp64 slots of every flow and clip
        assert fwd - ragged >= b * t * 4 + nfl * b * lib.fwn_ragged_logdet_slots(b) * 8
    assert lib.fwn_ragged_forward_workspace_bytes(C.byref(m), 1, 60) == 0          # T not a multiple of hop


def test_score_cropping_and_grouping():
    # hop 256 divides by 2^n_block = 256: nothing to crop
    assert [SC.cropped_frames(f, hparams) for f in (1, 3, 862)] == [1, 3, 862]
    # hop 8 against 2^5: four frames per unit - crop DOWN (synthesize pads up; a score must not invent samples)
    hp = small_hparams(n_block=5, hop_size=8, upsample_scales=[2, 4])
    assert [SC.cropped_frames(f, hp) for f in (1, 3, 4, 5, 9, 16)] == [0, 0, 4, 4, 8, 16]
    frames = [9, 3, 16, 4, 5, 1, 17]
    kept, groups = SC.plan(frames, 8, 0.25, hp)
    assert kept == [0, 2, 3, 4, 6]                                                     # the two short ones are dropped
    assert sorted(k for g in groups for k in g) == list(range(len(kept)))             # every kept utterance exactly once
    own = [SC.cropped_frames(frames[k], hp) for k in kept]
    assert groups == S.plan_batches(own, 8, 0.25, hp)
    for g in groups:
        top = max(own[k] for k in g)
        assert len(g) * top - sum(own[k] for k in g) <= 0.25 * len(g) * top
    assert SC.plan(frames, 1, 0.25, hp)[1] == [[k] for k in sorted(range(len(kept)), key=lambda k: (own[k], frames[kept[k]], k))]
    assert SC.plan([], 8, 0.25, hp) == ([], [])


def test_score_reads_train_txt_and_has_the_flags(tmp_path, monkeypatch):
    (tmp_path / "train.txt").write_text("dataset-audio-00001.npy|dataset-mel-00001.npy|768|0|some text\n"
                                        "dataset-audio-00002.npy|dataset-mel-00002.npy|1280|0|with | a bar\n\n", encoding="utf-8")
    assert SC.read_metadata(str(tmp_path)) == [("dataset-audio-00001.npy", "dataset-mel-00001.npy"),
                                               ("dataset-audio-00002.npy", "dataset-mel-00002.npy")]
    seen = {}
    monkeypatch.setattr(SC, "score", lambda args, hp: seen.update(vars(args)))
    SC.main(["--saved_dir", "ck", "--base_dir", "data", "--out", "s.jsonl", "--batch", "4", "--max_pad_frac", "0.1"])
    assert seen == dict(saved_dir="ck", base_dir="data", out="s.jsonl", batch=4, max_pad_frac=0.1)
    SC.main([])
    assert seen["batch"] == 8 and seen["max_pad_frac"] == 0.25
