"""Windowed synthesis on the GPU (-m gpu): the three kernels around the pass bit for bit against what they restate,
``reverse_windowed`` / ``synthesize_windowed`` / ``stream`` against the fp64 oracle's WHOLE-clip reverse, and the CLI's ``--window``.

What is held to what.  That the halo is exact is proved in fp64 on the CPU (tests/test_windowed_host.py: 1e-12); a halo a little
too small would leak 1e-5 .. 1e-13, which no bf16 pass shows.  These tests catch what the device path adds: offsets, seams,
stream positions.  Waveforms: the suite's ``ABS_WAV * max(1, |x0|max)`` (tests/test_gpu_parity.py) against the oracle's reverse
of the whole clip - and the same call with ``halo=0`` must EXCEED it (the control: this test sees a seam).  Latent: bit for bit
the slice of ``fwn_latent_normal`` where that slice fits a test (starts up to the unit); at starts of 2^32 + 6 and 2^34 - L the
whole-clip buffer would be 16 - 64 GiB, so those rows are held to the start-offset restatement of tests/philox_ref.py below
within its 1e-5 temp, and bit for bit to each other across a 2-sample shift of the start.  Copies and PCM: bit for bit.
"""
import ctypes as C
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402
import test_windowed_host as H  # noqa: E402

from oracle import flowavenet_np as onp  # noqa: E402
from tf_flowavenet_amd import _lib  # noqa: E402
from tf_flowavenet_amd import weights as W  # noqa: E402
from tf_flowavenet_amd import windowing as WIN  # noqa: E402
from tf_flowavenet_amd.model import FloWaveNet  # noqa: E402

from conftest import small_hparams  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABS_WAV = 1e-2
SEED = (1 << 32) + 75                         # the high key word is live
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i64(vals):
    return torch.tensor(list(vals), dtype=torch.int64).cuda()


def _i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32).cuda()


def _ids_dev(ids):
    return torch.from_numpy(np.asarray(ids, dtype=np.uint32).view(np.int32)).cuda()


# ---- fwn_latent_normal_at -------------------------------------------------------------------------------------------
def latent_at_ref(seed, clip_id, start, n, temp=1.0):
    """tests/philox_ref.py's ``latent_normal`` with a start: samples start .. start + n of the clip's stream, float64 [n]."""
    seed = int(seed) % (1 << 64)
    q0, q1 = int(start) // 4, (int(start) + int(n) + 3) // 4
    r = P.philox4x32_10((np.arange(q0, q1, dtype=np.uint64), 0, int(clip_id) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, seed >> 32))
    out = np.empty((q1 - q0, 4), dtype=np.float64)
    for pair in range(2):
        u1 = ((r[2 * pair] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (r[2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pair] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u2)
    off = int(start) - 4 * q0
    return out.reshape(-1)[off:off + int(n)] * float(temp)


def _latent_at(starts, ids, length, temp, lens=None, offset=0):
    """fwn_latent_normal_at into a NaN-prefilled [n, length] inside 7.5 sentinels, ``offset`` floats off 16 bytes -> float32 [n, length]."""
    lib = _lib.load()
    n = len(starts)
    buf = torch.full((GUARD + offset + n * length + GUARD,), 7.5, dtype=torch.float32, device="cuda")
    buf[GUARD + offset:GUARD + offset + n * length] = float("nan")
    assert buf.data_ptr() % 16 == 0
    sd, idd = _i64(starts), None if ids is None else _ids_dev(ids)
    ld = None if lens is None else _i32(lens)
    rc = lib.fwn_latent_normal_at(buf.data_ptr() + 4 * (GUARD + offset), n, length, SEED, None if idd is None else idd.data_ptr(),
                                  sd.data_ptr(), temp, None if ld is None else ld.data_ptr(), None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD + offset] == 7.5).all() and (got[GUARD + offset + n * length:] == 7.5).all()      # nothing outside [0, n L)
    body = got[GUARD + offset:GUARD + offset + n * length].reshape(n, length).copy()
    assert not np.isnan(body).any()                                                                      # and every sample inside
    return body


def _latent_whole(ids, t, temp):
    lib = _lib.load()
    z = torch.empty(len(ids), t, dtype=torch.float32, device="cuda")
    idd = _ids_dev(ids)
    assert lib.fwn_latent_normal(z.data_ptr(), len(ids), t, SEED, idd.data_ptr(), temp, None, None) == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    return z.cpu().numpy()


@pytest.mark.parametrize("length", [1, 7, 1030, 4100])
def test_latent_at_is_the_slice_of_fwn_latent_normal_bit_for_bit(length):
    temp, unit = 0.7, 16
    starts = [0, 4, 6, 1, unit, 5000 + 3]                          # rows with different starts and clip ids in one call
    ids = [0, 7, (1 << 32) - 1, 12345, 7, 3]
    whole = _latent_whole(ids, max(starts) + length, temp)
    for offset in (0, 1, 3):                                       # the buffer on and off a 16-byte boundary
        got = _latent_at(starts, ids, length, temp, offset=offset)
        for row, s in enumerate(starts):
            assert np.array_equal(_bits(got[row]), _bits(whole[row, s:s + length])), (length, offset, row, s)
    assert np.array_equal(_bits(_latent_at([0, 4, 6], None, length, temp)),                                 # NULL ids: clip r
                          _bits(np.stack([_latent_whole([0, 1, 2], 6 + length, temp)[r, s:s + length] for r, s in enumerate([0, 4, 6])])))


def test_latent_at_far_starts_match_the_restatement():
    length, temp = 1030, 0.7
    far = [(1 << 32) + 6, (1 << 32) + 4, (1 << 34) - length, (1 << 34) - length - 2, 0, 6]
    ids = [7, 7, 12345, 12345, 7, 7]
    got = _latent_at(far, ids, length, temp)
    for row, s in enumerate(far):
        ref = latent_at_ref(SEED, ids[row], s, length, temp)
        err = float(np.abs(got[row] - ref).max())
        print("start %d: max err %.3e (bound %.1e)" % (s, err, 1e-5 * temp))
        assert err <= 1e-5 * temp, (s, err)
    # a start shifted by two samples is the same stream, bit for bit (neither of the pair is a multiple of 4 apart from the even one)
    assert np.array_equal(_bits(got[0, :-2]), _bits(got[1, 2:]))
    assert np.array_equal(_bits(got[2, :-2]), _bits(got[3, 2:]))
    assert not np.array_equal(_bits(got[0]), _bits(got[5]))                     # 2^32 + 6 is not 6: the counter is the quad, not i mod 2^32
    assert np.array_equal(_bits(got[4, 6:]), _bits(got[5, :-6]))


def test_latent_at_lengths_clamp_to_plus_zero():
    length, temp = 1030, 1.0
    starts, ids = [6, 1, 16, (1 << 32) + 6], [0, 7, 3, 7]
    plain = _latent_at(starts, ids, length, temp)
    for offset in (0, 3):
        for lens in ([0, 5, 1030, 2000], [1029, 4, -3, 513]):                   # inside a quad, at the end, past it (clamped), negative
            got = _latent_at(starts, ids, length, temp, lens=lens, offset=offset)
            for row, n in enumerate(lens):
                n = min(max(n, 0), length)
                assert np.array_equal(_bits(got[row, :n]), _bits(plain[row, :n])), (lens, row)
                assert not _bits(got[row, n:]).any(), (lens, row)                # +0.0: every bit clear


# ---- fwn_window_gather / fwn_window_scatter_pcm16 ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_src():
    """One flat fp32 buffer of 2^31 + 2^20 elements, never filled: the tests touch only the rows they address."""
    buf = torch.empty((1 << 31) + (1 << 20), dtype=torch.float32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("row_floats", [8, 16, 80])
def test_window_gather_equals_numpy(row_floats, big_src):
    lib = _lib.load()
    rows = 37
    count = rows * row_floats
    top = ((1 << 31) + (1 << 19)) // row_floats                    # a row offset whose element offset is past 2^31
    src_rows = [0, 40, top, top + 3 * rows, 129]                   # disjoint spans of 37 rows each
    rng = np.random.default_rng(row_floats)
    want = rng.standard_normal((len(src_rows), count)).astype(np.float32)
    for sbase, dbase in ((0, 0), (1, 0), (0, 3), (2, 2)):          # source / destination on and off 16 bytes (in floats)
        src = big_src[sbase:]
        for r, s in enumerate(src_rows):
            src[s * row_floats:s * row_floats + count] = dev(want[r])
        out = torch.full((GUARD + dbase + len(src_rows) * count + GUARD,), 7.5, dtype=torch.float32, device="cuda")
        sd = _i64(src_rows)
        rc = lib.fwn_window_gather(src.data_ptr(), sd.data_ptr(), out.data_ptr() + 4 * (GUARD + dbase), len(src_rows), rows, row_floats, None)
        assert rc == 0, lib.fwn_last_error()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:GUARD + dbase] == 7.5).all() and (got[GUARD + dbase + want.size:] == 7.5).all()
        assert np.array_equal(_bits(got[GUARD + dbase:GUARD + dbase + want.size]), _bits(want.reshape(-1))), (row_floats, sbase, dbase)


def _pcm_values():
    f32 = np.float32
    special = [1.0, -1.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23, np.inf, -np.inf, 0.0, -0.0, 1e-40, 1.0 - 2.0 ** -24, 3.0, -3.0, np.nan]
    ks = np.concatenate([np.arange(0, 100), np.arange(16300, 16400), np.arange(32700, 32767)]).astype(np.float64)
    tie = ((ks + 0.5) / 32767.0).astype(f32)                       # the fp32 nearest every tie, and its two neighbours
    ties = np.concatenate([tie, np.nextafter(tie, f32(2.0)), np.nextafter(tie, f32(-2.0))])
    draws = (0.5 * np.random.default_rng(11).standard_normal(2048)).astype(f32)
    return np.concatenate([np.asarray(special, dtype=f32), ties, -ties, draws])


def _pcm16_dev(x):
    """fwn_pcm16 of float32 [n] -> int16 [n]: the arithmetic the scatter must reproduce (NaN -> 0 included)."""
    lib = _lib.load()
    xd, out = dev(x.astype(np.float32)), torch.empty(x.size, dtype=torch.int16, device="cuda")
    assert lib.fwn_pcm16(xd.data_ptr(), out.data_ptr(), 1, x.size, None, None) == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_window_scatter_equals_fwn_pcm16_and_writes_nothing_else():
    lib = _lib.load()
    length = 1031
    x = np.resize(_pcm_values(), (5, length)).astype(np.float32)
    x[3] = x[3, ::-1]
    far = (1 << 31) + 4096                                          # an output offset past 2^31 elements
    pcm = torch.empty(far + 4096, dtype=torch.int16, device="cuda")
    wav = torch.empty(far + 4096, dtype=torch.float32, device="cuda")
    core_off = [0, 3, 8, 1030, 100]
    core_len = [1031, 1000, 17, 1, 0]                               # the whole row, misaligned, short, one sample, nothing
    for obase in (0, 1, 5, 8):                                      # the destination's phase; x's rows are off 16 bytes (1031 odd) anyway
        out_off = [obase + 64, obase + 3000, far + obase, obase + 6000, obase + 7000]
        for o, n in zip(out_off, core_len):
            pcm[o - GUARD:o + n + GUARD] = 77
            wav[o - GUARD:o + n + GUARD] = 7.5
        for xoff in (0, 1):
            xd = torch.zeros(xoff + x.size, dtype=torch.float32, device="cuda")
            xd[xoff:] = dev(x.reshape(-1))
            offs, lens, outs = _i32(core_off), _i32(core_len), _i64(out_off)           # (held: the kernel reads them)
            for with_wav in (True, False):
                rc = lib.fwn_window_scatter_pcm16(xd.data_ptr() + 4 * xoff, 5, length, offs.data_ptr(), lens.data_ptr(), outs.data_ptr(),
                                                  pcm.data_ptr(), wav.data_ptr() if with_wav else None, None)
                assert rc == 0, lib.fwn_last_error()
            torch.cuda.synchronize()
            for r, (o, n) in enumerate(zip(out_off, core_len)):
                core = x[r, core_off[r]:core_off[r] + n]
                gp, gw = pcm[o - GUARD:o + n + GUARD].cpu().numpy(), wav[o - GUARD:o + n + GUARD].cpu().numpy()
                assert (gp[:GUARD] == 77).all() and (gp[GUARD + n:] == 77).all(), (obase, xoff, r)       # sentinels around every core
                assert (gw[:GUARD] == 7.5).all() and (gw[GUARD + n:] == 7.5).all(), (obase, xoff, r)
                if n:
                    assert np.array_equal(gp[GUARD:GUARD + n], _pcm16_dev(core)), (obase, xoff, r)
                    assert np.array_equal(gp[GUARD:GUARD + n], P.pcm16(np.nan_to_num(core, nan=0.0, posinf=np.inf, neginf=-np.inf)))
                    assert np.array_equal(_bits(gw[GUARD:GUARD + n]), _bits(core)), (obase, xoff, r)
    # a core that leaves its row is clamped into it on the device: nothing is read past x
    pcm[:4096] = 77
    xd, offs, lens, outs = dev(x.reshape(-1)), _i32([1000, -5, 2000, 0, 0]), _i32([500, 10, 10, -1, 0]), _i64([64, 1000, 2000, 3000, 3500])
    rc = lib.fwn_window_scatter_pcm16(xd.data_ptr(), 5, length, offs.data_ptr(), lens.data_ptr(), outs.data_ptr(), pcm.data_ptr(), None, None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    got = pcm[:4096].cpu().numpy()
    assert np.array_equal(got[64:95], _pcm16_dev(x[0, 1000:])) and (got[95:1000] == 77).all()
    assert np.array_equal(got[1000:1010], _pcm16_dev(x[1, :10])) and (got[1010:] == 77).all()
    del pcm, wav
    torch.cuda.empty_cache()


def test_window_entries_refuse_bad_arguments():
    lib = _lib.load()
    buf = torch.empty(4096, dtype=torch.float32, device="cuda")
    tab = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, t = buf.data_ptr(), tab.data_ptr()
    assert lib.fwn_latent_normal_at(None, 1, 8, 75, None, t, 1.0, None, None) == -1 and b"fwn_latent_normal_at" in lib.fwn_last_error()
    assert lib.fwn_latent_normal_at(p, 1, 8, 75, None, None, 1.0, None, None) == -1
    assert lib.fwn_latent_normal_at(p, 0, 8, 75, None, t, 1.0, None, None) == -1
    assert lib.fwn_latent_normal_at(p + 2, 1, 8, 75, None, t, 1.0, None, None) == -1
    assert lib.fwn_latent_normal_at(p, 1, 8, 75, None, t + 4, 1.0, None, None) == -1 and b"8-byte" in lib.fwn_last_error()
    assert lib.fwn_window_gather(None, t, p, 1, 2, 8, None) == -1 and b"fwn_window_gather" in lib.fwn_last_error()
    assert lib.fwn_window_gather(p, None, p + 1024, 1, 2, 8, None) == -1
    assert lib.fwn_window_gather(p, t + 4, p + 1024, 1, 2, 8, None) == -1
    assert lib.fwn_window_gather(p, t, p + 1024, 1, 0, 8, None) == -1
    assert lib.fwn_window_gather(p, t, p + 1024, 1, 1 << 20, 1 << 12, None) == -1
    assert lib.fwn_window_scatter_pcm16(p, 1, 8, t, t, t, None, None, None) == -1 and b"fwn_window_scatter_pcm16" in lib.fwn_last_error()
    assert lib.fwn_window_scatter_pcm16(p, 1, 8, t, t, t + 4, p + 1024, None, None) == -1
    assert lib.fwn_window_scatter_pcm16(p, 1, 8, t + 2, t, t, p + 1024, None, None) == -1
    assert lib.fwn_window_scatter_pcm16(p, 1, 8, t, t, t, p + 1025, None, None) == -1
    # the whole-group entry: before anything is launched
    hp = small_hparams()
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    fp8 = FloWaveNet(hp, gate_fp8=True).load_params(W.synthetic_params(hp, 99, actnorm="random"))
    md = C.byref(model._packed.model_desc)
    n = lib.fwn_synthesize_windows_workspace_bytes(md, 2, 64)
    assert n > lib.fwn_workspace_bytes(md, 2, 64) and lib.fwn_synthesize_windows_workspace_bytes(md, 0, 64) == 0
    assert lib.fwn_synthesize_windows_workspace_bytes(md, 2, 72) == 0                  # no multiple of hop
    assert lib.fwn_synthesize_windows_workspace_bytes(C.byref(fp8._packed.model_desc), 2, 64) > 0      # rectangular: fp8 gates keep working
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
    mel = torch.rand(64, hp.num_mels, device="cuda")
    pcm = torch.full((256,), 77, dtype=torch.int16, device="cuda")
    t32 = t + 256

    def call(m=md, mel_p=mel.data_ptr(), rows=t, ids=t32, starts=t, offs=t32, lens=t32, outs=t, w=wsp, wn=n, out=pcm.data_ptr()):
        return lib.fwn_model_synthesize_windows(m, 2, 64, mel_p, rows, ids, starts, offs, lens, outs, 75, 1.0, w, wn, out, None, None)

    for bad in (dict(m=None), dict(mel_p=None), dict(rows=None), dict(ids=None), dict(starts=None), dict(offs=None), dict(lens=None),
                dict(outs=None), dict(w=None), dict(out=None), dict(rows=t + 4), dict(starts=t + 4), dict(outs=t + 4), dict(ids=t32 + 2),
                dict(offs=t32 + 1), dict(lens=t32 + 2), dict(w=wsp + 16), dict(out=pcm.data_ptr() + 1)):
        assert call(**bad) == -1, bad
    assert call(wn=1024) == -3
    torch.cuda.synchronize()
    assert (pcm == 77).all()                                       # the refused calls launched nothing; core_len 0 writes nothing
    assert call() == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    assert (pcm == 77).all()


# ---- reverse_windowed against the oracle's whole-clip reverse ------------------------------------------------------------
_MODELS = {}


def _model(cfg, units):
    key = repr(cfg)
    if key not in _MODELS:
        case = H.oracle_inputs(cfg, units)
        _MODELS[key] = FloWaveNet(case["hp"]).load_params(case["params"])
    return _MODELS[key]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cfg,units", H.GEOMETRIES)
def test_reverse_windowed_matches_the_oracle_whole_clip_reverse(cfg, units, batch):
    """The clip, the plan and the weights of the fp64 stitching proof (tests/test_windowed_host.py).  Measured on an MI355X, err /
    bound per geometry: 0.0076 / 0.0170, 0.030 / 0.079, 0.065 / 0.143, 0.109 / 0.247, 0.127 / 0.241; the whole-clip ``reverse``
    of the same clip has 0.0076, 0.030, 0.065, 0.109, 0.141 (windowed against whole-clip ``reverse``: 0 in the first three
    geometries, at most 0.07 in the last two, where the call shapes take other dispatch forms: two realisations of the same
    bf16 rounding noise); halo 0: 0.60, 3.9, 5.5, 9.3, 7.6.  The bound is about the pass as much as about the windows: on the
    SECOND clip of ``W.synthetic_inputs(hp, 2, t)`` at the 8k geometry the whole-clip ``reverse`` itself is 0.337 off at one
    sample (bound 0.250; windowed: 0.280) - these loud weights at |x|max 25 over 3 264 samples, nothing a window adds.
    Clips of several ids pooled into one call are test_synthesize_windowed_end_to_end's."""
    case = H.oracle_inputs(cfg, units)
    model = _model(cfg, units)
    zd, cd = dev(case["z"]), dev(case["c"])
    x = model.reverse_windowed(zd, cd, case["window"], batch=batch)
    assert x.shape == (1, case["t"], 1) and x.dtype == torch.float32
    x0 = case["whole"]
    bound = ABS_WAV * max(1.0, float(np.abs(x0).max()))
    err = float(np.abs(x.cpu().numpy()[:, :, 0] - x0).max())
    cut = model.reverse_windowed(zd, cd, case["window"], batch=batch, halo=0)
    err_cut = float(np.abs(cut.cpu().numpy()[:, :, 0] - x0).max())
    print("%r batch %d: windowed err %.3e, halo 0 err %.3e (bound %.3e)" % (cfg, batch, err, err_cut, bound))
    assert err <= bound, (cfg, batch, err, bound)
    assert err_cut > bound, (cfg, batch, err_cut, bound)            # the control: a seam is seen
    assert torch.equal(x, model.reverse_windowed(zd, cd, case["window"], batch=batch))       # the same calls: the same bits


# ---- synthesize_windowed --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,units", [H.GEOMETRIES[0], H.GEOMETRIES[4]])
def test_synthesize_windowed_end_to_end(cfg, units):
    case = H.oracle_inputs(cfg, units)
    hp, t, window = case["hp"], case["t"], case["window"]
    model = _model(cfg, units)
    ids, temp = [12345, (1 << 32) - 1], float(hp.temp)
    c2 = W.synthetic_inputs(hp, 2, t, want=("c",))["c"].astype(np.float32)          # two clips: windows of both share calls
    cd = dev(c2)
    pcm, wav = model.synthesize_windowed(cd, SEED, clip_ids=ids, window=window, batch=3, return_wav=True)
    assert pcm.dtype == torch.int16 and pcm.shape == (2, t) and wav.shape == (2, t, 1)
    assert torch.equal(model.synthesize_windowed(cd, SEED, clip_ids=ids, window=window, batch=3), pcm)
    pcm_h, wav_h = pcm.cpu().numpy(), wav.cpu().numpy()[:, :, 0]
    assert np.array_equal(pcm_h, P.pcm16(wav_h))                    # the PCM is pcm16 of the returned waveform, exactly
    # the latent is sample_z's: the same windows run from it by reverse_windowed give the same waveform bit for bit,
    # and fwn_latent_normal_at over the plan's starts is its slices
    z = model.sample_z(2, t, SEED, clip_ids=ids)
    assert torch.equal(model.reverse_windowed(z, cd, window, batch=3), wav)
    plan = WIN.plan_windows(t, window, hp)
    lo, hi = plan[len(plan) // 2][:2]
    lib = _lib.load()
    zw = torch.empty(2, hi - lo, dtype=torch.float32, device="cuda")
    idd, sd = _ids_dev(ids), _i64([lo, lo])
    assert lib.fwn_latent_normal_at(zw.data_ptr(), 2, hi - lo, SEED, idd.data_ptr(), sd.data_ptr(), temp, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(zw, z[:, lo:hi, 0])
    # against the oracle's reverse of the fp64 Philox latent, whole clip
    z64 = P.latent_batch(SEED, ids, t, temp)
    x0 = onp.reverse(case["p64"], z64[:, :, None], c2.astype(np.float64), hp)[:, :, 0]
    bound = ABS_WAV * max(1.0, float(np.abs(x0).max()))
    err = float(np.abs(wav_h - x0).max())
    other = model.synthesize_windowed(cd, SEED, clip_ids=ids, window=2 * window, batch=8, return_wav=True)[1].cpu().numpy()[:, :, 0]
    err2 = float(np.abs(other - x0).max())
    cut = model.synthesize_windowed(cd, SEED, clip_ids=ids, window=window, batch=3, return_wav=True, halo=0)[1].cpu().numpy()[:, :, 0]
    err_cut = float(np.abs(cut - x0).max())
    print("%r: wav err %.3e, at twice the window %.3e, halo 0 %.3e (bound %.3e)" % (cfg, err, err2, err_cut, bound))
    assert err <= bound and err2 <= bound, (cfg, err, err2, bound)
    assert err_cut > bound, (cfg, err_cut, bound)
    with pytest.raises(ValueError):
        model.synthesize_windowed(cd, SEED, window=window + 1)
    with pytest.raises(ValueError):
        model.synthesize_windowed(cd, SEED, clip_ids=[0], window=window)


# ---- the full model -------------------------------------------------------------------------------------------------
def test_full_model_windowed_matches_the_golden_10s_clip():
    """BASELINE configs[3] (one 10 s clip, T = 220 672) at window 65 536 against the committed fp64 ``x_rev``, ActNorm initialised
    by the golden's own forward - the case and the bounds of test_baseline_configs_at_their_real_sizes_match_golden."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    name = "full_b8f6_T220672_10s"
    over, b, t, actnorm, ddi = mg.CASES[name]
    hp = mg.hp_of(over)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    half_ulp = 2.0 ** -11 if g["z"].dtype == np.float16 else 0.0
    model = FloWaveNet(hp, init=True).load_params(W.synthetic_params(hp, 1234, actnorm=actnorm))
    inp = W.synthetic_inputs(hp, b, t)
    c = dev(inp["c"])
    model.forward(dev(inp["x"]), c)                                 # the data-dependent ActNorm init
    plan = WIN.plan_windows(t, 65536, hp)
    assert len(plan) == 4 and WIN.halo_samples(hp) == 15872
    wav = model.reverse_windowed(dev(inp["z"]), c, 65536).cpu().numpy()
    x0 = g["x_rev"].astype(np.float32)
    assert wav.shape == x0.shape == (b, t, 1)
    scale = max(1.0, float(np.abs(x0).max()))
    print("max err %.3e (bound %.3e), mean err %.3e (bound %.3e)" % (np.abs(wav - x0).max(), ABS_WAV * scale, np.abs(wav - x0).mean(), 1e-3 * scale))
    assert (np.abs(wav - x0) <= ABS_WAV * scale + half_ulp * np.abs(x0)).all(), np.abs(wav - x0).max()
    assert np.abs(wav - x0).mean() < 1e-3 * scale


# ---- past what one call can address ---------------------------------------------------------------------------------------
def test_a_clip_past_the_ceiling_is_synthesized_and_exact_at_its_seams():
    hp = small_hparams()
    unit, h, window = WIN.unit_samples(hp), WIN.halo_samples(hp), 262144
    t = 4194304 + 16 * unit
    params = H.loud_params(hp)
    p64 = onp.to_f64(params)
    model = FloWaveNet(hp).load_params(params)
    c = torch.rand(1, t // hp.hop_size, hp.num_mels, generator=torch.Generator().manual_seed(3)).cuda()
    with pytest.raises(_lib.FwnError, match="exceeds"):
        model.synthesize(c, SEED, clip_ids=[7])
    pcm, wav = model.synthesize_windowed(c, SEED, clip_ids=[7], window=window, return_wav=True)
    assert pcm.shape == (1, t)
    assert torch.equal(pcm[0].cpu(), torch.from_numpy(P.pcm16(wav.cpu().numpy()[0, :, 0]).astype(np.int16)))
    seam = round(t / 2 / window) * window
    temp = float(hp.temp)
    for a in (0, seam - 2 * unit, t - 4 * unit):                    # clip start, across the seam nearest the middle, clip end
        b = a + 4 * unit
        lo, hi = max(0, a - h), min(t, b + h)
        z = latent_at_ref(SEED, 7, lo, hi - lo, temp)
        cw = c[0, lo // hp.hop_size:hi // hp.hop_size].cpu().numpy().astype(np.float64)
        x0 = onp.reverse(p64, z[None, :, None], cw[None], hp)[0, a - lo:b - lo, 0]
        got = wav[0, a:b, 0].cpu().numpy()
        bound = ABS_WAV * max(1.0, float(np.abs(x0).max()))
        err = float(np.abs(got - x0).max())
        print("span [%d, %d): err %.3e (bound %.3e)" % (a, b, err, bound))
        assert err <= bound, (a, err, bound)
        assert float(np.abs(got).max()) > 0.0


# ---- stream -----------------------------------------------------------------------------------------------------------
def test_stream_equals_synthesize_windowed_bit_for_bit():
    case = H.oracle_inputs(*H.GEOMETRIES[0])
    hp = case["hp"]
    model = _model(*H.GEOMETRIES[0])
    h, hop, window = WIN.halo_samples(hp), hp.hop_size, 256
    frames = 150
    c = torch.rand(1, frames, hp.num_mels, generator=torch.Generator().manual_seed(5)).cuda()
    want = model.synthesize_windowed(c, SEED, clip_ids=[9], window=window, batch=1)[0]
    first = (window + h) // hop                                     # the frame whose arrival completes the first window
    outs = {}
    for size in (1, 7, 64):
        for run in range(2 if size == 7 else 1):
            st = model.stream(SEED, clip_id=9, window=window)
            parts, arrived, first_at = [], 0, None
            while arrived < frames:
                f = min(size, frames - arrived)
                part = st.push(c[0, arrived:arrived + f] if size != 7 else c[0, arrived:arrived + f].cpu().numpy())
                assert part.dtype == torch.int16 and part.dim() == 1
                arrived += f
                if part.numel() and first_at is None:
                    first_at = arrived
                assert st.retained_frames <= (window + 2 * h) // hop + size
                parts.append(part)
            assert first_at is not None and first_at - size < first <= first_at, (size, first_at, first)
            parts.append(st.finish())
            outs[(size, run)] = torch.cat(parts)
            assert torch.equal(outs[(size, run)], want), size
    assert torch.equal(outs[(7, 0)], outs[(7, 1)])                  # two streams with the same arguments
    st = model.stream(SEED, window=window)
    st.push(c[0, :3])
    assert st.finish().shape == (48,)                               # shorter than one window: one window at finish
    hp5 = small_hparams(n_block=5)                                  # unit 32: two frames
    st = FloWaveNet(hp5).load_params(W.synthetic_params(hp5, 99, actnorm="random")).stream(SEED, window=64)
    st.push(torch.rand(3, hp5.num_mels))
    with pytest.raises(ValueError):
        st.finish()


# ---- the CLI ----------------------------------------------------------------------------------------------------------
CLIPS = (("a", 40), ("b", 6), ("c", 262144 + 40))                 # two short ones (not windowed), and one past what one call addresses
WINDOW = 65536


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    root = tmp_path_factory.mktemp("cliw")
    hp = small_hparams()
    params = H.loud_params(hp)
    (root / "ckpt").mkdir()
    (root / "mels").mkdir()
    np.savez(root / "ckpt" / "flowavenet_model.npz", **params)
    rng = np.random.default_rng(0)
    mels = {}
    for name, frames in CLIPS:
        mels[name] = rng.random((frames, hp.num_mels), dtype=np.float32)
        np.save(root / "mels" / (name + ".npy"), mels[name])
    return root, hp, params, mels


def _read(path, rate):
    with wave.open(str(path)) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, rate)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("device_rng", [False, True])
def test_synthesize_cli_window(cli_case, device_rng):
    from tf_flowavenet_amd import synthesize as S
    root, hp, params, mels = cli_case
    out = root / ("out_%d" % device_rng)
    base = dict(saved_dir=str(root / "ckpt"), mels_dir=str(root / "mels"), seed=75, batch=4, device_rng=device_rng)
    with pytest.raises(ValueError, match="exceeds"):                # without the flag clip c is what it was: too long for one call
        S.synthesize(type("A", (), dict(output_dir=str(root / "no"), **base))(), hp)
    args = type("A", (), dict(output_dir=str(out), window=WINDOW - 7, **base))()    # rounded up to WINDOW
    assert S.synthesize(args, hp) == ["a.npy", "b.npy", "c.npy"]
    model = FloWaveNet(hp).load_params(params)
    hop = hp.hop_size
    gen = torch.Generator(device="cpu").manual_seed(75)             # the default path's one generator, clips in ascending length
    for k, (name, frames) in sorted(enumerate(CLIPS), key=lambda e: e[1][1]):
        got = _read(out / (name + ".wav"), hp.sample_rate)
        assert got.size == frames * hop
        c = dev(mels[name][None])
        if frames * hop <= WINDOW:                                  # not windowed: the paths of before, the clip ids of before
            if device_rng:
                want = model.synthesize(c, 75, clip_ids=[k])[0].cpu().numpy()
            else:
                z = torch.randn(1, frames * hop, 1, generator=gen) * hp.temp
                want = P.pcm16(model.reverse(z.cuda(), c).cpu().numpy()[0, :, 0])
        elif device_rng:
            want = model.synthesize_windowed(c, 75, clip_ids=[k], window=WINDOW, batch=4)[0].cpu().numpy()
        else:
            z = torch.randn(1, frames * hop, 1, generator=torch.Generator(device="cpu").manual_seed(75 + k)) * hp.temp
            want = P.pcm16(model.reverse_windowed(z.cuda(), c, WINDOW, batch=4).cpu().numpy()[0, :, 0])
        assert np.array_equal(got, want), (name, device_rng)
        assert np.abs(got).max() > 0
