"""Host checks of windowed synthesis (no GPU): the halo formula, and - in fp64, with the NumPy oracle - that the inverse pass
run window by window over ``windowing.plan_windows`` and stitched core by core IS the whole-clip pass; the plans, the grouping,
the stream planner and the CLI flag.

Bounds.  Stitching: 1e-12 max(1, |x|max) - the halo covers the network's receptive field, so the only difference is fp64
summation order inside the oracle's convolutions (measured: at most 2.5e-14).  Negative control: the same with halo 0 must
exceed the suite's waveform bound 1e-2 max(1, |x|max) (measured: 23 - 85 times that) - a GPU test at that bound sees a seam."""
import numpy as np
import pytest

from oracle import flowavenet_np as onp
from tf_flowavenet_amd import synthesize as S
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd import windowing as WIN
from tf_flowavenet_amd.hparams import default_hparams, hparams8000

from conftest import small_hparams

# the five geometries of tests/test_ragged.py, each with the window (in units) its plan uses: 1 - 5 units
GEOMETRIES = [
    (dict(), 1),
    (dict(n_block=4, n_flow=2), 2),
    (dict(n_block=2, n_flow=4, n_layer=4), 3),
    (dict(n_block=5, n_flow=2, num_mels=16, hop_size=32, upsample_scales=[4, 8]), 4),
    ("8k", 5),
]


def hp_of(cfg):
    return hparams8000().replace(n_flow=2, num_mels=16) if cfg == "8k" else small_hparams(**cfg)


def loud_params(hp):
    """``W.synthetic_params(hp, 99, actnorm="random")`` with the ZeroConv kernels times 5 (tests/test_ragged.py): the coupling
    then depends on the WaveNet's output strongly enough that a wrong row shows far above the bound."""
    params = W.synthetic_params(hp, 99, actnorm="random")
    return {k: (v * 5.0).astype(v.dtype) if "/ZeroConv1d/" in k and k.endswith("kernel") else v for k, v in params.items()}


def case_shape(hp, units):
    """(T, window) of a geometry's test clip: T = 2 H + 3 window + unit, so the plan has a first window (clamped left), middle
    ones, a last core of (2 H + unit) % window samples where that is not 0 (short in three of the five geometries), and
    windows clamped right."""
    unit, h = WIN.unit_samples(hp), WIN.halo_samples(hp)
    window = units * unit
    return 2 * h + 3 * window + unit, window


def stitched(reverse, z, c, t, window, hp, halo=None):
    """reverse(z_window, c_window) -> x_window over the plan, cores copied: float64 [T]."""
    out = np.full(t, np.nan)
    for lo, hi, a, b in WIN.plan_windows(t, window, hp, halo):
        out[a:b] = reverse(z[lo:hi], c[lo // hp.hop_size:hi // hp.hop_size])[a - lo:b - lo]
    return out


_CASES = {}


def oracle_inputs(cfg, units):
    """Once per geometry, never changed: one clip's z and c (float32 [1, ...], as a model takes them), the loud parameters, and
    the fp64 oracle's whole-clip reverse [1, T].  tests/test_windowed.py holds the GPU paths to the same arrays."""
    key = repr(cfg)
    if key not in _CASES:
        hp = hp_of(cfg)
        t, window = case_shape(hp, units)
        params = loud_params(hp)
        p64 = onp.to_f64(params)
        inp = W.synthetic_inputs(hp, 1, t, want=("c", "z"))
        z, c = inp["z"].astype(np.float32), inp["c"].astype(np.float32)
        whole = onp.reverse(p64, z.astype(np.float64), c.astype(np.float64), hp)[:, :, 0]
        _CASES[key] = dict(hp=hp, t=t, window=window, params=params, p64=p64, z=z, c=c, whole=whole)
    return _CASES[key]


def oracle_case(cfg, units):
    """``oracle_inputs`` plus, for clip 0, the oracle's stitched reverse with the halo and with none."""
    case = oracle_inputs(cfg, units)
    if "halo" not in case:
        hp, t, window = case["hp"], case["t"], case["window"]
        z, c = case["z"][0, :, 0].astype(np.float64), case["c"][0].astype(np.float64)

        def rev(zw, cw):
            return onp.reverse(case["p64"], zw[None, :, None], cw[None], hp)[0, :, 0]

        case["halo"] = stitched(rev, z, c, t, window, hp)
        case["cut"] = stitched(rev, z, c, t, window, hp, halo=0)
    return case


def test_halo_values():
    assert WIN.halo_samples(default_hparams()) == 15872 and WIN.unit_samples(default_hparams()) == 256
    assert WIN.halo_samples(hparams8000()) == 2112 and WIN.unit_samples(hparams8000()) == 96
    assert WIN.halo_samples(small_hparams()) == 96 and WIN.unit_samples(small_hparams()) == 16
    for cfg, _ in GEOMETRIES:
        hp = hp_of(cfg)
        unit = int(np.lcm(hp.hop_size, 1 << hp.n_block))
        reach = 1 + sum(3 ** layer for layer in range(hp.n_layer))
        raw = hp.n_flow * reach * (2 ** (hp.n_block + 1) - 2) + 2 * hp.hop_size
        h = WIN.halo_samples(hp)
        assert WIN.unit_samples(hp) == unit and h % unit == 0 and raw <= h < raw + unit, (cfg, h, raw, unit)


@pytest.mark.parametrize("cfg,units", GEOMETRIES)
def test_stitched_oracle_reverse_is_the_whole_clip_reverse(cfg, units):
    case = oracle_case(cfg, units)
    plan = WIN.plan_windows(case["t"], case["window"], case["hp"])
    h, t = WIN.halo_samples(case["hp"]), case["t"]
    assert plan[0][0] == 0 and plan[0][1] < t                                   # first: clamped left only
    assert any(lo > 0 and hi < t and hi - lo == case["window"] + 2 * h for lo, hi, _, _ in plan)      # a middle one
    assert plan[-1][3] - plan[-1][2] == (t % case["window"] or case["window"])  # the last core: what is left (short where T % window)
    assert sum(1 for lo, hi, _, b in plan if hi == t and b + h > t) >= 2        # clamped right, more than the last
    whole = case["whole"][0]
    scale = max(1.0, float(np.abs(whole).max()))
    err = float(np.abs(case["halo"] - whole).max())
    print("%r: T %d window %d halo %d: stitched - whole %.3e (bound %.1e)" % (cfg, t, case["window"], h, err, 1e-12 * scale))
    assert np.isfinite(case["halo"]).all()
    assert err <= 1e-12 * scale, (cfg, err)


@pytest.mark.parametrize("cfg,units", GEOMETRIES)
def test_without_a_halo_the_seams_show_far_above_the_waveform_bound(cfg, units):
    case = oracle_case(cfg, units)
    whole = case["whole"][0]
    bound = 1e-2 * max(1.0, float(np.abs(whole).max()))
    err = float(np.abs(case["cut"] - whole).max())
    print("%r: halo 0: stitched - whole %.3e = %.1f x the bound %.3e" % (cfg, err, err / bound, bound))
    assert err > bound, (cfg, err, bound)


def test_plan_properties():
    for cfg, _ in GEOMETRIES + [("stock", 0)]:
        hp = default_hparams() if cfg == "stock" else hp_of(cfg)
        unit, h = WIN.unit_samples(hp), WIN.halo_samples(hp)
        for window in (unit, 3 * unit, 7 * unit):
            for t in (unit, window, window + unit, 2 * h + 3 * window + unit, 5 * window):
                for halo in (None, 0, 2 * unit):
                    hh = h if halo is None else halo
                    plan = WIN.plan_windows(t, window, hp, halo)
                    assert len(plan) == -(-t // window)
                    edge = 0
                    for lo, hi, a, b in plan:
                        assert a == edge and a < b <= t and b - a <= window          # the cores tile [0, t) in order
                        assert lo == max(0, a - hh) and hi == min(t, b + hh)         # the clamps
                        assert not (lo % unit or hi % unit or a % unit or b % unit)
                        edge = b
                    assert edge == t
                    assert all(b - a == window for _, _, a, b in plan[:-1])
                    if t <= window:
                        assert plan == [(0, t, 0, t)]                             # one window, no halo
    hp = small_hparams()
    for bad in (0, -16, 8, 24, 16.5):
        with pytest.raises(ValueError):
            WIN.plan_windows(256, bad, hp)
    for bad in (-16, 8, 24):
        with pytest.raises(ValueError):
            WIN.plan_windows(256, 32, hp, halo=bad)
    for bad in (0, 8, 250):
        with pytest.raises(ValueError):
            WIN.plan_windows(bad, 32, hp)


def test_grouping():
    hp = small_hparams()                              # unit 16, H 96
    plans = [WIN.plan_windows(t, 64, hp) for t in (64 * 9 + 16, 64 * 6, 48)]
    for batch in (1, 3, 8):
        groups = WIN.group_windows(plans, batch)
        seen = [m for g in groups for m in g]
        assert sorted(seen) == [(clip, k) for clip, plan in enumerate(plans) for k in range(len(plan))]     # every window once
        for g in groups:
            assert 1 <= len(g) <= batch
            assert len({plans[clip][k][1] - plans[clip][k][0] for clip, k in g}) == 1                     # one length per call
        by_len = {}
        for g in groups:
            clip, k = g[0]
            by_len.setdefault(plans[clip][k][1] - plans[clip][k][0], []).append(len(g))
        for sizes in by_len.values():
            assert all(s == batch for s in sizes[:-1])                                                     # full calls first
    # one long clip: the first window, the middle ones, and the end - a handful of shapes whatever its length
    for t in (128 * 40, 128 * 400 + 16):              # (window >= H; a shorter window ramps over several windows at both ends)
        plan = WIN.plan_windows(t, 128, hp)
        assert len({hi - lo for lo, hi, _, _ in plan}) <= 4
    # windows of several clips are pooled: the middle windows of clips 0 and 1 share calls
    groups = WIN.group_windows(plans, 8)
    assert any(len({clip for clip, _ in g}) > 1 for g in groups)
    with pytest.raises(ValueError):
        WIN.group_windows(plans, 0)
    # with hparams, a call also stays inside what one inverse pass addresses (synthesize.max_clips_per_call's rule)
    stock = default_hparams()
    assert WIN.max_windows_per_call(stock, 1048576 + 2 * 15872) == S.max_clips_per_call(stock, 1048576 + 2 * 15872) == 3
    plan = WIN.plan_windows(8 * 1048576, 1048576, stock)
    assert max(len(g) for g in WIN.group_windows([plan], 8, stock)) == 3 and max(len(g) for g in WIN.group_windows([plan], 8)) == 6
    with pytest.raises(ValueError, match="smaller window"):
        WIN.group_windows([WIN.plan_windows(2 * 4194304, 4194304, stock)], 8, stock)


def test_stream_planner():
    hp = small_hparams()                              # hop 16, unit 16, H 96
    h, hop, window = WIN.halo_samples(hp), hp.hop_size, 64
    frames = (2 * h + 5 * window + 16) // hop
    want = WIN.plan_windows(frames * hop, window, hp)
    for split in ([1] * frames, [7] * (frames // 7) + [frames % 7], [frames], [3, 0, 11] + [2] * ((frames - 14) // 2) + [(frames - 14) % 2]):
        assert sum(split) == frames
        sp = WIN.StreamPlanner(hp, window)
        got, arrived, kept_most = [], 0, 0
        for f in split:
            before = sp.first_frame
            out = sp.push(f)
            arrived += f
            kept_most = max(kept_most, arrived - before)            # frames held while this push is served
            for lo, hi, a, b in out:
                need = (b + h) // hop                              # core k is released exactly when frame (b_k + H) / hop is in
                assert arrived - f < need <= arrived, (split[:3], a, need, arrived)
            got += out
        assert all((b + h) // hop > arrived for _, _, a, b in want[len(got):])         # nothing computable is held back
        rest = sp.finish()
        assert got + rest == want, split[:3]                      # any split releases the same windows; finish flushes
        assert kept_most <= (window + 2 * h) // hop + max(split)
        with pytest.raises(ValueError):
            sp.push(1)
    # a clip shorter than one window: nothing until finish, then the single window without a halo
    sp = WIN.StreamPlanner(hp, 64)
    assert sp.push(3) == [] and sp.finish() == [(0, 48, 0, 48)]
    # the frame total must be a multiple of unit / hop
    hp2 = small_hparams(n_block=5)                    # unit 32 = two frames
    sp = WIN.StreamPlanner(hp2, 64)
    sp.push(3)
    with pytest.raises(ValueError):
        sp.finish()
    with pytest.raises(ValueError):
        WIN.StreamPlanner(hp, 24)


class _StreamModel:
    """Stands in for FloWaveNet under ``SynthesisStream``: the device call writes each core's absolute sample indices into the
    PCM buffer and records (absolute start, length, core); frame f of the mel holds f, so a window names the frames it was given."""

    def __init__(self, hp):
        self._hparams, self._device, self.hop = hp, "cpu", hp.hop_size
        self.windows = []

    @staticmethod
    def _clip_id_values(clip_ids, b):
        return [int(v) for v in clip_ids]

    def _windows_call(self, mel_flat, rows, length, seed, temp, pcm_flat, wav_flat):
        import torch
        (clip_id, start, mel_row, core_off, core_len, out_off), = rows
        assert clip_id == 7 and seed == 75 and temp == 0.5 and out_off == 0 and wav_flat is None
        assert mel_row >= 0 and mel_row + length // self.hop <= mel_flat.shape[0]
        frames = mel_flat[mel_row:mel_row + length // self.hop, 0]
        assert np.array_equal(frames.numpy() * self.hop, np.arange(start, start + length, self.hop))   # the window's own frames
        assert pcm_flat.numel() == core_len
        pcm_flat[:] = torch.arange(start + core_off, start + core_off + core_len, dtype=torch.int16)
        self.windows.append((start, length, core_off, core_len))


def test_synthesis_stream_bookkeeping():
    """The twin of tests/test_windowed_forward_host.py ``test_stream_bookkeeping``: the same clip, window and splits."""
    import torch
    from tf_flowavenet_amd.model import SynthesisStream
    hp = small_hparams()                              # hop 16, unit 16, H 96
    h, hop, window = WIN.halo_samples(hp), hp.hop_size, 64
    frames = (2 * h + 5 * window + 16) // hop
    t = frames * hop
    c = (torch.arange(frames, dtype=torch.float32)[:, None]).repeat(1, hp.num_mels)
    plan = WIN.plan_windows(t, window, hp)
    for split in ([1] * frames, [7] * (frames // 7) + [frames % 7], [frames], [3, 0, 11] + [2] * ((frames - 14) // 2) + [(frames - 14) % 2]):
        model = _StreamModel(hp)
        ss = SynthesisStream(model, 75, 7, window, temp=0.5)
        got, at = [], 0
        for f in split:
            got.append(ss.push(c[at:at + f]))
            at += f
            assert ss.retained_frames <= (window + 2 * h) // hop + max(split)
        got.append(ss.finish())
        assert all(g.dtype == torch.int16 for g in got)
        assert torch.equal(torch.cat(got), torch.arange(t, dtype=torch.int16))       # every core once, in order, whatever the split
        assert [(lo, hi - lo, a - lo, b - a) for lo, hi, a, b in plan] == model.windows
    # frames of another width are refused; the total must be a multiple of the unit
    ss = SynthesisStream(_StreamModel(hp), 75, 7, window, temp=0.5)
    with pytest.raises(ValueError):
        ss.push(c[:2, :3])
    hp5 = small_hparams(n_block=5)                    # unit 32 = two frames
    ss = SynthesisStream(_StreamModel(hp5), 75, 7, 64)
    ss.push(c[:3])
    with pytest.raises(ValueError):
        ss.finish()


def test_upload_tables():
    """One buffer, the int64 columns first: every pointer aligned for its type, every column the values put in - negative
    int32 and uint32 ids from 2^31 on alike."""
    import ctypes
    from tf_flowavenet_amd import windowed
    for n in (1, 5):
        cols64 = [[(1 << 40) + 3 * i for i in range(n)], [-(1 << 35) - i for i in range(n)], [i for i in range(n)]]
        cols32 = [[-1 - i for i in range(n)], [(1 << 31) + 5 * i for i in range(n)], [(1 << 32) - 1 - i for i in range(n)],
                  [-(1 << 31) + i for i in range(n)], [7 * i for i in range(n)]]
        tab, p64, p32 = windowed.upload_tables(cols64, cols32, "cpu")
        assert tab.numel() == n * (8 * len(cols64) + 4 * len(cols32)) and len(p64) == len(cols64) and len(p32) == len(cols32)
        assert p64[0] == tab.data_ptr() and all(p % 8 == 0 for p in p64) and all(p % 4 == 0 for p in p32)
        spans = sorted([(p, 8 * n) for p in p64] + [(p, 4 * n) for p in p32])
        assert all(p + size <= q for (p, size), (q, _) in zip(spans, spans[1:]))            # no column overlaps another
        assert spans[-1][0] + spans[-1][1] == tab.data_ptr() + tab.numel()
        for p, col in zip(p64, cols64):
            assert list((ctypes.c_int64 * n).from_address(p)) == col
        for p, col in zip(p32, cols32):
            assert list((ctypes.c_uint32 * n).from_address(p)) == [v % (1 << 32) for v in col]
            assert [v for v in (ctypes.c_int32 * n).from_address(p)] == [(v + (1 << 31)) % (1 << 32) - (1 << 31) for v in col]


def test_cli_window_flag(monkeypatch, tmp_path):
    from tf_flowavenet_amd.hparams import hparams
    seen = []
    with monkeypatch.context() as mp:
        mp.setattr(S, "synthesize", lambda args, hp: seen.append(vars(args)))
        S.main([])
        S.main(["--window", "65000", "--device_rng"])
    assert "window" not in seen[0]                                  # off by default: the namespace is what it was
    assert seen[1]["window"] == 65000 and seen[1]["device_rng"] is True
    assert S.window_samples(65000, hparams) == 65024 and S.window_samples(65536, hparams) == 65536       # rounded up to 256
    assert S.window_samples(1, small_hparams()) == 16
    with pytest.raises(ValueError):
        S.window_samples(0, hparams)


def test_without_the_flag_synthesize_takes_none_of_the_new_code(monkeypatch, tmp_path):
    """The default CLI path with every windowed entry replaced by one that raises: it must not notice."""
    import torch

    def boom(*a, **k):
        raise AssertionError("windowed code reached without --window")

    for name in ("_synthesize_windowed", "window_samples"):
        monkeypatch.setattr(S, name, boom)
    for name in ("plan_windows", "group_windows", "halo_samples", "unit_samples", "StreamPlanner"):
        monkeypatch.setattr(WIN, name, boom)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)          # no device here: the model below is a stand-in

    class Model:
        reverse_windowed = synthesize_windowed = stream = boom

        def reverse(self, z, c, lengths=None):
            return torch.zeros(z.shape[0], z.shape[1], 1)

    hp = small_hparams()
    (tmp_path / "mels").mkdir()
    for name, frames in (("a", 5), ("b", 3)):
        np.save(tmp_path / "mels" / (name + ".npy"), np.zeros((frames, hp.num_mels), dtype=np.float32))
    for extra in (dict(), dict(ragged=True, max_pad_frac=0.5)):
        args = type("A", (), dict(mels_dir=str(tmp_path / "mels"), output_dir=str(tmp_path / "out"), seed=1, batch=2, **extra))()
        assert S.synthesize(args, hp, model=Model()) == ["a.npy", "b.npy"]
        assert (tmp_path / "out" / "a.wav").stat().st_size == 44 + 2 * 5 * hp.hop_size
