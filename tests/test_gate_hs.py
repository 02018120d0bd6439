"""The register-streamed hoisted gate (csrc/cond_rs.h gate_hs_kernel): the gate with a precomputed conditioning projection P at
the row counts where the ring path runs its un-split 64 x 128 tile (3 009 - 6 016 rows; inference hoists below 4 096).  It reads
Wd from a fragment stream (fwn_flow_desc.Wds) and must give the ring tile's bits: same MFMAs per output element in the same
order, same epilogue expression."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import _lib, packing
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd.model import FloWaveNet

pytestmark = pytest.mark.gpu

# every instantiation of the kernel: (rows, columns) of the workgroup tile
TILES = [(64, 512), (96, 512), (128, 512), (64, 256), (96, 256), (128, 256)]
# (clips, rows per clip): bottom of the range with a ragged last tile; a clip edge inside almost every tile; block 4 of the
# 8-clip pass; one clip just below the hoisting limit
SHAPES = [(1, 3009), (48, 63), (8, 504), (1, 4095)]
BLK = 4


def _hp5():
    return default_hparams().replace(n_block=5, n_flow=2)


@pytest.fixture(scope="module")
def twins():
    """The 5-block model whose block 4 has 4 032 rows at 8 x 16 128, packed with and without the Wd streams, both after the
    same data-dependent init pass."""
    hp = _hp5()
    inp = W.synthetic_inputs(hp, 8, 16128)
    x, c, z = (torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in ("x", "c", "z"))
    models = []
    for stream in (True, False):
        m = FloWaveNet(hp, init=True, gate_hs_stream=stream).load_params(W.synthetic_params(hp, 1234))
        m.forward(x, c)
        models.append(m)
    torch.cuda.synchronize()
    return hp, models[0], models[1], x, c, z


def _operands(m, seed, zero=None):
    rng = np.random.default_rng(seed)
    h = torch.from_numpy(rng.standard_normal((m, 256)).astype(np.float32) * 0.5).cuda().to(torch.bfloat16)
    P = torch.from_numpy(rng.standard_normal((m, 512)).astype(np.float32)).cuda()
    if zero == "P":
        P.zero_()
    if zero == "h":
        h.zero_()
    return h, P


def _gate(lib, d, layer, h, P, m, ti, tile=None):
    """o of fwn_gate (tile None) or of fwn_gate_tile on the named tile, with 8 guard rows behind the matrix."""
    o = torch.full((m + 8, 256), 7.0, device="cuda", dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    if tile is None:
        _lib.check(lib.fwn_gate(C.byref(d), layer, h.data_ptr(), None, P.data_ptr(), o.data_ptr(), m, ti, st), "fwn_gate")
    else:
        n = lib.fwn_gate_tile(C.byref(d), layer, h.data_ptr(), P.data_ptr(), o.data_ptr(), m, ti, tile[0], tile[1], st)
        assert n == -(-m // tile[0]) * (512 // tile[1]), (n, lib.fwn_last_error())
    assert bool((o[m:] == 7.0).all()), "the kernel wrote past row M"
    return o[:m]


def _descs(twins):
    hp, model, plain, _, _, _ = twins
    d = model._packed.flow_descs[BLK * hp.n_flow]
    d_plain = _lib.FlowDesc.from_buffer_copy(d)
    for l in range(_lib.FWN_MAX_LAYERS):
        d_plain.Wds[l] = None
    assert all(d.Wds[l] for l in range(hp.n_layer)) and not any(plain._packed.flow_descs[BLK * hp.n_flow].Wds[l] for l in range(hp.n_layer))
    return d, d_plain


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("b,ti", SHAPES)
def test_streamed_hoisted_gate_equals_the_ring_tile_bit_for_bit(twins, b, ti, layer):
    """fwn_gate with the descriptor's Wd stream, and every instantiated tile through fwn_gate_tile, against fwn_gate on a
    descriptor copy with the stream pointer NULL (the ring path's 64 x 128 tile): both dilations, same operands and P."""
    lib = _lib.load()
    d, d_plain = _descs(twins)
    m = b * ti
    h, P = _operands(m, 100 * b + layer)
    want = _gate(lib, d_plain, layer, h, P, m, ti)
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0.1
    # the call really takes the streamed form at this shape: the shipped tile has fewer workgroups than the ring tile's 4 ceil(M / 64)
    n = lib.fwn_gate_tile(C.byref(d), layer, h.data_ptr(), P.data_ptr(), torch.empty_like(want).data_ptr(), m, ti, 0, 0,
                          torch.cuda.current_stream().cuda_stream)
    assert 0 < n < 4 * -(-m // 64), n
    assert torch.equal(_gate(lib, d, layer, h, P, m, ti), want)
    for tile in TILES:
        assert torch.equal(_gate(lib, d, layer, h, P, m, ti, tile), want), tile


@pytest.mark.parametrize("zero", ["P", "h"])
def test_the_two_sums_of_the_streamed_hoisted_gate_separately(twins, zero):
    """P all zeros (only bias + taps @ Wd), h all zeros (only bias + P): each sum alone equals the ring tile's."""
    lib = _lib.load()
    d, d_plain = _descs(twins)
    b, ti, layer = 48, 63, 1
    m = b * ti
    h, P = _operands(m, 7, zero)
    want = _gate(lib, d_plain, layer, h, P, m, ti)
    assert torch.equal(_gate(lib, d, layer, h, P, m, ti), want)
    for tile in TILES:
        assert torch.equal(_gate(lib, d, layer, h, P, m, ti, tile), want), tile


@pytest.mark.parametrize("layer", [0, 1])
def test_streamed_hoisted_gate_matches_the_fp64_oracle(twins, layer):
    """Every instantiation against the oracle's ResBlock gate (modules.py:113-124) at 48 clips of 63 rows, at
    test_gate_stage_kernel_matches_oracle's tolerance.  P holds the conditioning term in the device's units (packed-N columns,
    pre-multiplied by the exponent scales); the oracle adds the same values plus the conditioning convs' biases, which the
    device carries in its gate bias."""
    hp = twins[0]
    lib = _lib.load()
    d, _ = _descs(twins)
    b, ti = 48, 63
    m = b * ti
    h, P = _operands(m, 31 + layer)
    p64 = onp.to_f64(W.synthetic_params(hp, 1234))
    fg, gch = packing.gate_row_channel()
    P64 = P.cpu().numpy().astype(np.float64)
    pf = np.empty((m, 256))
    pg = np.empty((m, 256))
    pf[:, gch[fg == 0]] = P64[:, fg == 0] / packing.GATE_MUL[0]
    pg[:, gch[fg == 1]] = P64[:, fg == 1] / packing.GATE_MUL[1]
    h64 = h.float().cpu().numpy().astype(np.float64).reshape(b, ti, 256)
    rp = W.flow_prefix(BLK, 0) + "/WaveNet/ResBlock_%d" % layer
    f = onp.conv_layer(p64, rp + "/Conv_filter", h64, 3, 3 ** layer).reshape(m, 256) + pf + p64[rp + "/filter_conv_c/bias"].reshape(1, 256)
    g = onp.conv_layer(p64, rp + "/Conv_gate", h64, 3, 3 ** layer).reshape(m, 256) + pg + p64[rp + "/gate_conv_c/bias"].reshape(1, 256)
    want = np.tanh(f) * onp.sigmoid(g)
    for tile in [None] + TILES:
        err = np.abs(_gate(lib, d, layer, h, P, m, ti, tile).float().cpu().numpy() - want)
        # bf16 weights and a bf16 output in (-1, 1): half an output ulp is 2e-3, the weight rounding adds ~1e-2
        assert err.max() < 3e-2 and err.mean() < 2e-3, (tile, err.max(), err.mean(), np.unravel_index(err.argmax(), err.shape))


def test_whole_model_equals_its_twin_without_the_stream_and_on_three_streams(twins):
    """Forward and reverse of the 5-block model at 8 x 16 128 (block 4: 4 032 rows, hoisted) equal, bit for bit, the twin
    packed without the Wd streams; and the same passes issued on three streams at once equal the one-stream results."""
    hp, model, plain, x, c, z = twins
    ref_nll = torch.stack(model.forward(x, c)).clone()
    ref_wav = model.reverse(z, c).clone()
    assert torch.equal(torch.stack(plain.forward(x, c)), ref_nll)
    assert torch.equal(plain.reverse(z, c), ref_wav)
    torch.cuda.synchronize()
    lanes = [torch.cuda.Stream() for _ in range(3)]
    outs = []
    for k in range(6):
        with torch.cuda.stream(lanes[k % 3]):
            if k % 2:
                outs.append(("inv", model.reverse(z, c).clone()))
            else:
                outs.append(("fwd", torch.stack(model.forward(x, c)).clone()))
    torch.cuda.synchronize()
    for kind, got in outs:
        assert torch.equal(got, ref_wav if kind == "inv" else ref_nll), kind
