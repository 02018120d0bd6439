"""Gradient accumulation, the part that needs no GPU: the C entry refuses bad arguments before any launch, the block ranges
the per-range fold walks cover the flat layout, and the host-side admission rules of ``Trainer`` and ``train.py``."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import small_hparams
from tf_flowavenet_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_entry_is_declared_and_bound_with_its_five_arguments(lib):
    res, args = _lib.SIGNATURES["fwn_grad_accumulate"]
    assert len(args) == 5 and hasattr(lib, "fwn_grad_accumulate")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fwn.h")).read()
    assert "int fwn_grad_accumulate(float* dst, const float* a, const float* b, int64_t n, void* stream);" in header
    assert lib.fwn_version() == 322                     # additive: the version stays


def test_the_entry_refuses_bad_arguments_before_any_launch(lib):
    """FWN_ERR_ARG (-1) with a message naming the entry, on a machine without a GPU: nothing was launched."""
    A, B_, D = 1 << 20, 1 << 21, 1 << 22                # never dereferenced
    bad = [
        ((None, A, B_, 16), b"NULL"),                    # null dst
        ((D, A, None, 16), b"NULL"),                     # null b
        ((D, A, B_, 0), b"positive"),                    # n <= 0
        ((D, A, B_, -4), b"positive"),
        ((D + 2, A, B_, 16), b"4-byte"),                 # a pointer not 4-byte aligned: dst, a, b
        ((D, A + 1, B_, 16), b"4-byte"),
        ((D, None, B_ + 3, 16), b"4-byte"),
        ((D, D + 4, B_, 16), b"overlap"),                # partial overlap with a, from either side
        ((D, D - 4 * 15, B_, 16), b"overlap"),
        ((D, None, D + 4 * 15, 16), b"overlap"),         # ... and with b
        ((D, A, D - 4, 16), b"overlap"),
    ]
    for args, word in bad:
        assert lib.fwn_grad_accumulate(*args, None) == -1, args
        msg = lib.fwn_last_error()
        assert b"fwn_grad_accumulate" in msg and word in msg, (args, msg)


def test_block_ranges_cover_the_whole_flat_layout():
    """The fold of a pending sum runs range by range inside the block hook: together the ranges must be the layout - the
    up-sampling convs first, then one per block, back to back from 0 to the size."""
    from tf_flowavenet_amd.optim import DataParallelAdam
    from tf_flowavenet_amd.weights import FlatLayout
    from tf_flowavenet_amd.hparams import default_hparams
    for hp in (small_hparams(n_block=3, n_flow=2, n_layer=2, hop_size=16, upsample_scales=[4, 4], num_mels=16), default_hparams()):
        layout = FlatLayout(hp)
        ranges = DataParallelAdam.block_ranges(SimpleNamespace(layout=layout))
        assert [k for k, _, _ in ranges] == ["upsample"] + ["Block_%d" % i for i in range(hp.n_block)]
        assert ranges[0][1] == 0 and ranges[-1][2] == layout.size
        assert all(lo < hi for _, lo, hi in ranges)
        assert all(a[2] == b[1] for a, b in zip(ranges, ranges[1:]))


def test_a_micro_batch_of_another_size_is_refused_on_the_host_with_the_pending_state_untouched():
    from tf_flowavenet_amd.training import Trainer
    tr = SimpleNamespace(pending=2, _pending_b=4, engine=None)
    with pytest.raises(ValueError, match="clips"):
        Trainer._admit(tr, np.zeros((3, 256), np.float32), None)
    assert (tr.pending, tr._pending_b) == (2, 4)
    assert Trainer._admit(tr, np.zeros((4, 128), np.float32), None) is None       # another T is fine
    tr.pending = 0
    assert Trainer._admit(tr, np.zeros((3, 256), np.float32), None) is None       # nothing pending: any size starts an update


def test_train_cli_rejects_accum_steps_below_one(capsys):
    from tf_flowavenet_amd import train as TL
    for bad in ("0", "-2", "x"):
        with pytest.raises(SystemExit) as e:
            TL.main(["--accum_steps", bad])
        assert e.value.code == 2
    assert "--accum_steps" in capsys.readouterr().err
