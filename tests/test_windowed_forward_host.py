"""Host checks of the windowed forward (no GPU).  In fp64, with the NumPy oracle: the halo of ``windowing.halo_samples`` is the
forward pass's halo too - the latent stitched from the windows' cores IS the whole-clip latent - and per-clip ``log_p`` /
``logdet`` composed from CORE sums by the rule of tests/windowed_forward_ref.py are ``onp.forward``'s.  Then the CLI flag's
parsing and plan, and the stream's bookkeeping with the device call replaced.

Bounds.  Stitching: 1e-12 max(1, |z|max) and 1e-12 on the scalars - the only difference is fp64 summation order (measured: at
most 1.3e-13).  Negative controls with halo 0, against the suite's GPU bounds (tests/test_ragged_forward.py): z must miss
ABS_Z max(1, |z|max) on all five geometries (measured 10.9 - 36.5 times it); log_p must miss REL_LOGP on four of them (1.5e-2 -
4.9e-1) and does not on the n_block = 5 one (8.8e-4), which is asserted too so that nobody reads more into log_p than it sees."""
import json

import numpy as np
import pytest

from tf_flowavenet_amd import score as SC
from tf_flowavenet_amd import synthesize as S
from tf_flowavenet_amd import windowing as WIN
from tf_flowavenet_amd.hparams import default_hparams

from conftest import small_hparams
from test_windowed_host import GEOMETRIES
from windowed_forward_ref import oracle_case

REL_LOGP = 1e-3          # tests/test_ragged_forward.py's
ABS_Z = 2e-2
LOGP_BLIND = [cfg for cfg, _ in GEOMETRIES if isinstance(cfg, dict) and cfg.get("n_block") == 5]


@pytest.mark.parametrize("cfg,units", GEOMETRIES)
def test_stitched_oracle_forward_is_the_whole_clip_forward(cfg, units):
    case = oracle_case(cfg, units)
    lp, ld, z = case["halo"]
    scale = max(1.0, float(np.abs(case["z"]).max()))
    err = float(np.abs(z - case["z"]).max())
    print("%r: T %d window %d: stitched z - whole z %.3e (bound %.1e), log_p %.3e, logdet %.3e off"
          % (cfg, case["t"], case["window"], err, 1e-12 * scale, abs(lp - case["log_p"]), abs(ld - case["logdet"])))
    assert len(WIN.plan_windows(case["t"], case["window"], case["hp"])) >= 4
    assert np.isfinite(z).all()
    assert err <= 1e-12 * scale, (cfg, err)
    assert abs(lp - case["log_p"]) <= 1e-12, (cfg, lp, case["log_p"])
    assert abs(ld - case["logdet"]) <= 1e-12, (cfg, ld, case["logdet"])


@pytest.mark.parametrize("cfg,units", GEOMETRIES)
def test_without_a_halo_the_seams_show_far_above_the_bounds(cfg, units):
    case = oracle_case(cfg, units)
    lp, _, z = case["cut"]
    bound = ABS_Z * max(1.0, float(np.abs(case["z"]).max()))
    err = float(np.abs(z - case["z"]).max())
    rel = abs(lp - case["log_p"]) / abs(case["log_p"])
    print("%r: halo 0: z off by %.3e = %.1f x the bound %.3e; log_p off by %.3e relative" % (cfg, err, err / bound, bound, rel))
    assert err > bound, (cfg, err, bound)
    if cfg in LOGP_BLIND:
        assert rel <= REL_LOGP, (cfg, rel)           # the seams of this geometry are below what log_p resolves
    else:
        assert rel > REL_LOGP, (cfg, rel)


def test_only_one_geometry_is_blind():
    assert len(LOGP_BLIND) == 1


# ---------------------------------------------------------------------------------------------- score --window
def test_cli_window_flag(monkeypatch):
    from tf_flowavenet_amd.hparams import hparams
    seen = []
    with monkeypatch.context() as mp:
        mp.setattr(SC, "score", lambda args, hp: seen.append(vars(args)))
        SC.main([])
        SC.main(["--window", "65000", "--batch", "4"])
    assert "window" not in seen[0]                                  # off by default: the namespace is what it was
    assert seen[1]["window"] == 65000 and seen[1]["batch"] == 4
    assert S.window_samples(65000, hparams) == 65024


def test_windowed_plan():
    hp = small_hparams()                                            # hop 16, unit 16
    frames = [5, 40, 0, 12, 41, 8]
    long_ones, planned = SC.windowed_plan(frames, 192, hp)
    assert long_ones == {1, 4} and planned == frames                # 640 and 656 samples > 192 (12 frames are 192: not long)
    assert SC.windowed_plan(frames, 656, hp)[0] == set()            # "longer than", not "at least"
    assert SC.windowed_plan(frames, 640, hp)[0] == {4}
    # an utterance past what one call addresses is planned as absent - the ordinary plan would refuse it - and still long
    stock = default_hparams()
    big = (4194304 + 256) // stock.hop_size
    long_ones, planned = SC.windowed_plan([10, big, 300], 65536, stock)
    assert long_ones == {1, 2} and planned == [10, 0, 300]
    kept, groups = SC.plan(planned, 8, 0.25, stock)
    assert kept == [0, 2] and sorted(g for group in groups for g in group) == [0, 1]
    # n_block 5 with hop 16: the crop is to 32 samples = the unit
    hp5 = small_hparams(n_block=5)
    assert SC.cropped_frames(9, hp5) * hp5.hop_size == 128 and 128 % WIN.unit_samples(hp5) == 0


class _ScoreModel:
    """Stands in for FloWaveNet in ``score``: records the calls, returns each clip's length as its scalars."""

    def __init__(self):
        self.calls = []

    def forward(self, x, c, lengths=None):
        import torch
        self.calls.append(("forward", tuple(x.shape), list(lengths)))
        v = torch.tensor([float(n) for n in lengths])
        return v, -v

    def forward_windowed(self, x, c, window=None, batch=8):
        import torch
        self.calls.append(("windowed", tuple(x.shape), window, batch))
        v = torch.tensor([float(x.shape[1]) + 0.5])
        return v, -v


def _score_dir(tmp_path, hp, frame_counts):
    for sub in ("audios", "mels"):
        (tmp_path / sub).mkdir()
    lines = []
    for k, f in enumerate(frame_counts):
        np.save(tmp_path / "audios" / ("a%d.npy" % k), np.zeros(f * hp.hop_size, dtype=np.float32))
        np.save(tmp_path / "mels" / ("m%d.npy" % k), np.zeros((f, hp.num_mels), dtype=np.float32))
        lines.append("a%d.npy|m%d.npy|%d|0|text" % (k, k, f * hp.hop_size))
    (tmp_path / "train.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")


def test_score_window_keeps_every_other_call(monkeypatch, tmp_path):
    """With the device replaced: the long utterances go through ``forward_windowed``, cropped to the unit; every ``forward``
    call that holds a short utterance is the call a run without the flag makes - same members, same shape - and the records
    come out in train.txt's order."""
    import torch
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    hp = small_hparams(n_block=5)                                   # unit 32 = two frames
    counts = [4, 41, 6, 1, 40, 5]                                   # 1 frame: below the alignment, skipped either way
    _score_dir(tmp_path, hp, counts)
    runs = {}
    for name, extra in (("plain", dict()), ("window", dict(window=100))):
        model = _ScoreModel()
        args = type("A", (), dict(saved_dir="", base_dir=str(tmp_path), out=str(tmp_path / (name + ".jsonl")), batch=8,
                                  max_pad_frac=0.9, **extra))()
        recs = SC.score(args, hp, model=model)
        assert [json.loads(line) for line in (tmp_path / (name + ".jsonl")).read_text().splitlines()] == recs
        runs[name] = (model.calls, recs)
    plain_calls, plain = runs["plain"]
    calls, recs = runs["window"]
    assert all(c[0] == "forward" for c in plain_calls)
    windowed = [c for c in calls if c[0] == "windowed"]
    assert [c[1] for c in windowed] == [(1, 40 * 16, 1), (1, 40 * 16, 1)]       # 41 frames cropped to 40: a multiple of the unit
    assert all(c[2] == 128 and c[3] == 8 for c in windowed)                      # --window 100 rounded up to the unit
    kept_calls = [c for c in calls if c[0] == "forward"]
    assert kept_calls and all(c in plain_calls for c in kept_calls)              # no call of another shape or membership
    assert [r["name"] for r in recs] == [r["name"] for r in plain] == ["a0.npy", "a1.npy", "a2.npy", "a4.npy", "a5.npy"]
    for r, r0 in zip(recs, plain):
        if r["name"] in ("a1.npy", "a4.npy"):
            assert r["samples"] == 640 and r["log_p"] == 640.5 and r["nll"] == 0.0
        else:
            assert r == r0


def test_without_the_flag_score_takes_none_of_the_new_code(monkeypatch, tmp_path):
    import torch

    def boom(*a, **k):
        raise AssertionError("windowed code reached without --window")

    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    for name in ("windowed_plan", "window_samples"):
        monkeypatch.setattr(SC, name, boom)
    hp = small_hparams()
    _score_dir(tmp_path, hp, [4, 9])
    model = _ScoreModel()
    model.forward_windowed = boom
    args = type("A", (), dict(saved_dir="", base_dir=str(tmp_path), out=str(tmp_path / "s.jsonl"), batch=8, max_pad_frac=0.9))()
    assert [r["samples"] for r in SC.score(args, hp, model=model)] == [64, 144]


# ---------------------------------------------------------------------------------------------- the stream's bookkeeping
class _StreamModel:
    """Stands in for FloWaveNet under ``ForwardStream``: the device call copies each window's core of the audio into z and
    records (absolute start, length, core, slot); the finish returns the number of slots."""

    def __init__(self, hp):
        self._hparams, self._device, self.hop = hp, "cpu", hp.hop_size
        self.windows = []
        self.most = 0

    def _default_window(self):
        return 64

    def _forward_windows_call(self, x_flat, mel_flat, rows, length, acc, z_flat):
        (x_row, mel_row, core_off, core_len, slot, z_off), = rows
        assert x_row == mel_row and x_row >= 0 and (x_row + length // self.hop) <= x_flat.shape[0] == mel_flat.shape[0]
        assert acc.shape[0] > slot and z_off == 0
        audio = x_flat.reshape(-1)[x_row * self.hop:x_row * self.hop + length]
        frames = mel_flat[mel_row:mel_row + length // self.hop, 0]
        assert np.array_equal(audio[::self.hop].numpy(), frames.numpy() * self.hop)     # audio and mel stayed aligned
        z_flat[:core_len] = audio[core_off:core_off + core_len]
        self.windows.append((int(audio[0]), length, core_off, core_len, slot))

    def _forward_windows_finish(self, acc, slot0, nwin):
        import torch
        assert slot0 == [0]
        return torch.tensor([[float(nwin[0])], [-float(nwin[0])]])


def test_stream_bookkeeping():
    import torch
    from tf_flowavenet_amd.model import ForwardStream
    hp = small_hparams()                                            # hop 16, unit 16, H 96
    h, hop, window = WIN.halo_samples(hp), hp.hop_size, 64
    frames = (2 * h + 5 * window + 16) // hop
    t = frames * hop
    x = torch.arange(t, dtype=torch.float32)                        # sample i holds i: a z core names the samples it came from
    c = (torch.arange(frames, dtype=torch.float32)[:, None]).repeat(1, hp.num_mels)
    plan = WIN.plan_windows(t, window, hp)
    for split in ([1] * frames, [7] * (frames // 7) + [frames % 7], [frames], [3, 0, 11] + [2] * ((frames - 14) // 2) + [(frames - 14) % 2]):
        model = _StreamModel(hp)
        fs = ForwardStream(model, window)
        got, at = [], 0
        for f in split:
            got.append(fs.push(x[at * hop:(at + f) * hop], c[at:at + f]))
            at += f
            assert fs.retained_frames <= (window + 2 * h) // hop + max(split)
        z, lp, ld = fs.finish()
        got.append(z)
        assert torch.equal(torch.cat(got), x)                       # every core once, in order, whatever the split
        assert [(lo, hi - lo, a - lo, b - a, k) for k, (lo, hi, a, b) in enumerate(plan)] == model.windows
        assert float(lp) == len(plan) == -float(ld)
    # without return_z the pushes return nothing, the scalars still come
    model = _StreamModel(hp)
    model._forward_windows_call = lambda x_flat, mel_flat, rows, length, acc, z_flat: model.windows.append(z_flat)
    fs = ForwardStream(model, window, return_z=False)
    assert fs.push(x, c).numel() == 0
    z, lp, _ = fs.finish()
    assert z.numel() == 0 and float(lp) == len(plan) and all(w is None for w in model.windows)
    # samples and frames must match; the total must be a multiple of the unit; nothing pushed is an error
    fs = ForwardStream(_StreamModel(hp), window)
    with pytest.raises(ValueError):
        fs.push(x[:17], c[:1])
    with pytest.raises(ValueError):
        fs.finish()
    hp5 = small_hparams(n_block=5)                                  # unit 32 = two frames
    fs = ForwardStream(_StreamModel(hp5), 64)
    fs.push(x[:48], c[:3])
    with pytest.raises(ValueError):
        fs.finish()
