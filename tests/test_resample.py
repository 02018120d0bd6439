"""GPU tests of the sample-rate conversion: ``fwn_resample`` against the fp64 restatement (tests/resample_ref.py) at the fp32
dot-product bound, ragged batches and chunked clips bit for bit against one call, 64-bit positions, equal rates, ``preprocess``
on corpora that are not at the model's rate, and ``synthesize --out_rate``.

The bound.  An output is a dot product of K fp32 terms with coefficients rounded once from fp64: whatever the summation order,
with or without FMA, |y - y64| <= (K + 2) 2^-24 A[m], A[m] = sum |x[n] h[.]| (``resample_ref.bound``).  Inputs are
float32-representable, so they carry no error of their own."""
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref as R
from oracle import mel_np as onp
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd.model import FloWaveNet

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 22050), (44100, 22050), (22050, 8000), (16000, 22050), (22050, 48000), (96000, 8000)]
PCM_PAIRS = [(48000, 22050), (22050, 48000)]
TILE = 256                 # csrc/resample.hip: outputs per workgroup
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _tiles_plus_one(up, down):
    """The shortest clip with more than three tiles of outputs."""
    n = (3 * TILE * down) // up
    while R.n_out(n, up, down) < 3 * TILE + 1:
        n += 1
    return n


def _table(up, down):
    from tf_flowavenet_amd.resample import design_table
    return torch.from_numpy(design_table(up, down)).cuda()


def _run(lib, x, table, up, down, n_total, in_start=0, m0=0, n_out=None, lens=None):
    """fwn_resample of x [B, n_in] (float32 / int16 ndarray) -> float32 [B, n_out], through guard bands of 77 that must survive."""
    b, n_in = x.shape
    n_out = R.n_out(n_total, up, down) - m0 if n_out is None else n_out
    xd = torch.from_numpy(x).cuda()
    stride = n_out + 2 * GUARD
    y = torch.full((b * stride + GUARD,), 77.0, dtype=torch.float32, device="cuda")
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int64).cuda()
    rc = lib.fwn_resample(xd.data_ptr(), int(x.dtype == np.int16), b, n_in, in_start, n_in, None if ld is None else ld.data_ptr(),
                          n_total, table.data_ptr(), up, down, R.ZEROS, y.data_ptr() + 4 * GUARD, stride, m0, n_out, None)
    assert rc == 0, lib.fwn_last_error()
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.all(y[:GUARD] == 77.0)
    rows = y[GUARD:].reshape(b, stride)
    assert np.all(rows[:, n_out:] == 77.0), "a guard band was written"
    return rows[:, :n_out].copy()


def _check(got, x64, up, down, what, **at):
    """got [n] against the restatement of the clip x64 at the fp32 dot-product bound; -> the worst share of the bound."""
    m = at.pop("m", np.arange(len(got)))
    y, a, _ = R.resample_at(x64, up, down, m, **at)
    lim = R.bound(a, R.taps(up, down))
    err = np.abs(got.astype(np.float64) - y)
    share = float((err / np.maximum(lim, 1e-300)).max()) if len(got) else 0.0
    print("%s: max error %.3e, %.3f of the bound" % (what, float(err.max()) if len(got) else 0.0, share))
    assert np.all(err <= lim), (what, float(err.max()), share)
    return share


# ---- the kernel against the restatement ----

@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_kernel_matches_restatement_at_the_dot_product_bound(lib, in_rate, out_rate):
    up, down = R.ratio(in_rate, out_rate)
    table = _table(up, down)
    rng = np.random.default_rng(in_rate * 3 + out_rate)
    for n in (1, 7, 1000, _tiles_plus_one(up, down)):
        kinds = [np.float32] + ([np.int16] if (in_rate, out_rate) in PCM_PAIRS else [])
        for kind in kinds:
            if kind is np.float32:
                x = (rng.uniform(-1.0, 1.0, (3, n)) * np.array([[1.0], [0.01], [0.5]])).astype(np.float32)
                x64 = x.astype(np.float64)
            else:
                x = rng.integers(-32768, 32768, (3, n)).astype(np.int16)
                x64 = x.astype(np.float64) / 32768.0
            got = _run(lib, x, table, up, down, n)
            assert got.shape == (3, R.n_out(n, up, down))
            for b in range(3):
                _check(got[b], x64[b], up, down, "%d -> %d, n = %d, %s, row %d" % (in_rate, out_rate, n, kind.__name__, b))


# ---- ragged batches ----

@pytest.mark.parametrize("in_rate,out_rate", [(48000, 22050), (22050, 48000)])
def test_ragged_batch_gives_each_clip_what_it_gives_alone(in_rate, out_rate):
    from tf_flowavenet_amd.resample import Resampler
    rs = Resampler(in_rate, out_rate)
    t = 3000
    lens = [0, 1, 999, t]
    x = np.random.default_rng(9).uniform(-1.0, 1.0, (4, t)).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan                       # never loaded: a sample at or past a clip's end
    got = rs(torch.from_numpy(x), lengths=lens).cpu().numpy()
    assert got.shape == (4, rs.out_length(t)) and not np.isnan(got).any()
    dev = rs(torch.from_numpy(x), lengths=torch.tensor(lens).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), dev.view(np.uint32))
    for b, n in enumerate(lens):
        alone = rs(torch.from_numpy(x[b, :n].copy())).cpu().numpy()
        k = rs.out_length(n)
        assert alone.shape == (k,) and k == R.n_out(n, rs.up, rs.down)
        assert np.array_equal(got[b, :k].view(np.uint32), alone.view(np.uint32)), (b, n)
        assert np.all(got[b, k:].view(np.uint32) == 0)             # exact +0 past n_out(len)
        if n:
            _check(alone, x[b, :n].astype(np.float64), rs.up, rs.down, "alone, n = %d" % n)


# ---- chunking ----

def test_stream_equals_one_call_bit_for_bit():
    from tf_flowavenet_amd.resample import Resampler
    rs = Resampler(48000, 22050)
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, 50000).astype(np.float32)).cuda()
    whole = rs(x)
    for chunk in (1, 4096, 7777):
        s = rs.stream()
        parts = []
        for a in range(0, len(x), chunk):
            out = s.push(x[a:a + chunk])
            if out is not None:
                parts.append(out)
            assert s.retained <= rs.taps
        tail = s.finish()
        if tail is not None:
            parts.append(tail)
        got = torch.cat(parts)
        assert got.shape == whole.shape and torch.equal(got.view(torch.int32), whole.view(torch.int32)), chunk
        assert len(parts) > 1
    pcm = (x * 32767).to(torch.int16)
    s = rs.stream()
    got = torch.cat([p for p in [s.push(pcm[:20000]), s.push(pcm[20000:]), s.finish()] if p is not None])
    assert torch.equal(got.view(torch.int32), rs(pcm).view(torch.int32))


# ---- 64-bit arithmetic ----

def test_positions_past_2_to_the_32(lib):
    up, down = R.ratio(48000, 22050)
    hh, n_total, in_start, n_in = R.half_width(up, down), 1 << 33, (1 << 32) + 12345, 20000
    # the outputs whose whole support the span covers: ceil((m down - Hh) / up) >= in_start, floor((m down + Hh) / up) < in_start + n_in
    m_lo = ((in_start - 1) * up + hh) // down + 1
    m_hi = ((in_start + n_in) * up - hh - 1) // down
    assert m_hi - m_lo > 9000 and m_lo * down > 1 << 39           # m down, n up and n itself are all past 32 bits
    x = np.random.default_rng(33).uniform(-1.0, 1.0, (1, n_in)).astype(np.float32)
    table = _table(up, down)
    got = _run(lib, x, table, up, down, n_total, in_start=in_start, m0=m_lo, n_out=m_hi - m_lo + 1)
    _check(got[0], x[0].astype(np.float64), up, down, "clip of 2^33 samples, span at 2^32 + 12345",
           m=np.arange(m_lo, m_hi + 1), n_total=n_total, in_start=in_start)
    assert np.abs(got).max() > 0.1
    # one output more on either side reads a sample outside the span: refused before the launch
    xd, y = torch.from_numpy(x).cuda(), torch.empty(m_hi - m_lo + 2, device="cuda")
    for m0, n in ((m_lo - 1, 4), (m_hi - 2, 4)):
        assert lib.fwn_resample(xd.data_ptr(), 0, 1, n_in, in_start, n_in, None, n_total, table.data_ptr(), up, down, R.ZEROS,
                                y.data_ptr(), n, m0, n, None) == -1
        assert b"provided span" in lib.fwn_last_error()


# ---- equal rates ----

def test_equal_rates_return_the_values_without_a_launch():
    from tf_flowavenet_amd.resample import Resampler
    rs = Resampler(22050, 22050)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("equal rates called %s" % name)

    rs._lib = NoLaunch()
    x = torch.randn(2, 500)
    assert rs.out_length(500) == 500
    assert torch.equal(rs(x).cpu(), x) and torch.equal(rs(x[0]).cpu(), x[0])
    pcm = torch.randint(-32768, 32768, (2, 500), dtype=torch.int16)
    assert torch.equal(rs(pcm).cpu(), pcm.to(torch.float32) / 32768.0)
    got = rs(x, lengths=[100, 500]).cpu()
    assert torch.equal(got[0, :100], x[0, :100]) and torch.all(got[0, 100:] == 0) and torch.equal(got[1], x[1])


# ---- preprocess on corpora that are not at the model's rate ----

def _write_wav(path, rate, width, frames):
    frames = np.asarray(frames)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if frames.ndim == 1 else frames.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        flat = frames.reshape(-1)
        if width == 3:
            v = flat.astype(np.int64) & 0xFFFFFF
            w.writeframes(np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=1).astype(np.uint8).tobytes())
        else:
            w.writeframes(flat.astype("<i2").tobytes())


def _speechlike(seed, n, rate):
    t = np.arange(n) / float(rate)
    rng = np.random.default_rng(seed)
    return 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 1730.0 * t + 1.0) + 0.05 * rng.standard_normal(n)


def test_preprocess_resamples_a_corpus_of_other_rates(tmp_path):
    from tf_flowavenet_amd import preprocessing as P
    hp = default_hparams()
    book = tmp_path / "in" / "book1"
    os.makedirs(book / "wavs")
    a = np.stack([_speechlike(1, 21000, 48000), _speechlike(2, 21000, 48000)], axis=1)
    clips = [("u0", 48000, 3, np.round(a * 8388607.0).astype(np.int64), 8388608.0),             # 24-bit stereo
             ("u1", 48000, 2, np.round(_speechlike(3, 17321, 48000) * 32767.0).astype(np.int64), 32768.0),
             ("u2", 16000, 2, np.round(_speechlike(4, 7000, 16000) * 32767.0).astype(np.int64), 32768.0)]
    for name, rate, width, pcm, _ in clips:
        _write_wav(book / "wavs" / (name + ".wav"), rate, width, pcm)
    (book / "metadata.csv").write_text("\n".join("%s|t|t" % c[0] for c in clips), encoding="utf-8")
    out = tmp_path / "out"
    meta = P.preprocess(str(tmp_path / "in"), str(out), hp)
    assert len(meta) == 3
    hop = hp.hop_size
    for i, (name, rate, width, pcm, scale) in enumerate(clips):
        x = (pcm.astype(np.float64) / scale).astype(np.float32)          # exact: 16 and 24-bit values fit float32
        if x.ndim == 2:
            x = x.mean(axis=1)                                           # the channel mean, in float32 as read_wav takes it
        up, down = R.ratio(rate, hp.sample_rate)
        y64, amp, _ = R.resample(x.astype(np.float64), rate, hp.sample_rate)
        a0, m0 = onp.process_utterance(y64, hp)
        audio, mel = np.load(out / "audios" / ("dataset-audio-%05d.npy" % (i + 1))), np.load(out / "mels" / ("dataset-mel-%05d.npy" % (i + 1)))
        assert audio.dtype == mel.dtype == np.float32 and len(audio) == len(a0) == mel.shape[0] * hop and mel.shape == m0.shape
        assert mel.shape[0] == 1 + R.n_out(len(x), up, down) // hop
        # the resampler's bound, through the peak normalisation and the padding, plus test_mel.py's 1e-6
        gain = hp.rescaling_max / np.abs(y64).max()
        pad = (len(y64) // hop + 1) * hop - len(y64)
        lim = np.pad(R.bound(amp, R.taps(up, down)) * gain, (pad // 2, pad // 2 + pad % 2))[:len(a0)] + 1e-6
        err = np.abs(audio - a0)
        print("%s: audio max error %.2e (%.3f of its bound), mel max error %.2e"
              % (name, err.max(), (err / lim).max(), np.abs(mel - m0).max()))
        assert np.all(err <= lim), (name, err.max())
        assert np.abs(mel - m0).max() <= 2e-4 + 1e-5, name


def test_preprocess_at_the_models_rate_writes_the_same_bytes(tmp_path):
    """A corpus already at hparams.sample_rate: what read_wav -> _process_utterance -> np.save wrote before load_wav existed."""
    from tf_flowavenet_amd import preprocessing as P
    hp = default_hparams()
    book = tmp_path / "in" / "book1"
    os.makedirs(book / "wavs")
    sizes = (9000, 12345)
    for i, n in enumerate(sizes):
        _write_wav(book / "wavs" / ("u%d.wav" % i), hp.sample_rate, 2, np.round(_speechlike(10 + i, n, hp.sample_rate) * 32767.0))
    (book / "metadata.csv").write_text("\n".join("u%d|t|t %d" % (i, i) for i in range(2)), encoding="utf-8")
    out = tmp_path / "out"
    P.preprocess(str(tmp_path / "in"), str(out), hp)
    mel_fn = P.MelSpectrogram(hp)
    rows = []
    for i in range(2):
        audio, mel = P._process_utterance(P.read_wav(str(book / "wavs" / ("u%d.wav" % i)), hp.sample_rate), hp, mel_fn)
        for kind, arr in (("audio", audio), ("mel", mel)):
            ref = tmp_path / ("ref-%s.npy" % kind)
            np.save(ref, arr, allow_pickle=False)
            name = "dataset-%s-%05d.npy" % (kind, i + 1)
            assert (out / (kind + "s") / name).read_bytes() == ref.read_bytes(), name
        rows.append("dataset-audio-%05d.npy|dataset-mel-%05d.npy|%d|0|t %d" % (i + 1, i + 1, len(audio), i))
    assert (out / "train.txt").read_text(encoding="utf-8") == "\n".join(rows) + "\n"


# ---- synthesize --out_rate ----

CLIPS = (("a", 5), ("b", 3), ("c", 7), ("d", 5))


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    from tf_flowavenet_amd.hparams import hparams
    root = tmp_path_factory.mktemp("cli_rate")
    hp = hparams.replace(n_block=3, n_flow=2)
    params = W.synthetic_params(hp, 2, actnorm="random")
    (root / "ckpt").mkdir()
    (root / "mels").mkdir()
    np.savez(root / "ckpt" / "flowavenet_model.npz", **params)
    rng = np.random.default_rng(0)
    for name, frames in CLIPS:
        np.save(root / "mels" / (name + ".npy"), rng.random((frames, 80), dtype=np.float32))
    return root, hp, FloWaveNet(hp).load_params(params)


class _Recorder:
    """The model the CLI drives, keeping the float audio of every ``reverse`` call: the CLI's own z, the CLI's own batches."""

    def __init__(self, model):
        self._model, self.calls = model, []

    def reverse(self, *a, **kw):
        wav = self._model.reverse(*a, **kw)
        self.calls.append(wav.squeeze(-1).cpu().numpy().copy())
        return wav


def _args(root, out, **kw):
    base = dict(saved_dir=str(root / "ckpt"), mels_dir=str(root / "mels"), output_dir=str(out), seed=75, batch=4)
    base.update(kw)
    return type("A", (), base)()


def _read(path):
    with wave.open(str(path)) as w:
        assert (w.getnchannels(), w.getsampwidth()) == (1, 2)
        return w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("out_rate", [8000, 48000])
def test_synthesize_out_rate(cli_case, tmp_path, out_rate, ragged):
    from tf_flowavenet_amd import synthesize as S
    root, hp, model = cli_case
    names, frames = [n for n, _ in CLIPS], [f for _, f in CLIPS]
    extra = dict(ragged=True, max_pad_frac=0.5) if ragged else {}
    rec = _Recorder(model)
    S.synthesize(_args(root, tmp_path / "out", out_rate=out_rate, **extra), hp, rec)
    groups = S.plan_batches(frames, 4, 0.5, hp) if ragged else [[1], [0, 3], [2]]      # without: by length, ascending
    assert len(rec.calls) == len(groups)
    up, down = R.ratio(hp.sample_rate, out_rate)
    k = R.taps(up, down)
    for wav, group in zip(rec.calls, groups):
        for row, idx in enumerate(group):
            n = frames[idx] * hp.hop_size
            rate, pcm = _read(tmp_path / "out" / (names[idx] + ".wav"))
            assert rate == out_rate and len(pcm) == R.n_out(n, up, down)
            y64, amp, _ = R.resample(wav[row, :n].astype(np.float64), hp.sample_rate, out_rate)
            scaled = np.clip(y64, -1.0, 1.0) * 32767.0
            want = scaled.round().astype(np.int64)
            diff = np.abs(pcm.astype(np.int64) - want)
            assert diff.max() <= 1, (names[idx], int(diff.max()))
            # a sample may differ only where the fp64 value sits within the kernel's bound of a rounding boundary
            moved = diff > 0
            to_half = np.abs(np.abs(scaled - np.floor(scaled)) - 0.5)
            assert np.all(to_half[moved] <= R.bound(amp, k)[moved] * 32767.0), names[idx]
            print("%s -> %d Hz: %d of %d samples one LSB off" % (names[idx], out_rate, int(moved.sum()), len(pcm)))
            assert np.abs(pcm).max() > 0


def test_synthesize_without_the_flag_is_unchanged(cli_case, tmp_path):
    """No --out_rate: the bytes of write_wav over the CLI's own reverse calls, with and without --ragged."""
    from tf_flowavenet_amd import synthesize as S
    root, hp, model = cli_case
    names, frames = [n for n, _ in CLIPS], [f for _, f in CLIPS]
    for ragged in (False, True):
        extra = dict(ragged=True, max_pad_frac=0.5) if ragged else {}
        rec = _Recorder(model)
        out = tmp_path / ("out%d" % ragged)
        S.synthesize(_args(root, out, **extra), hp, rec)
        groups = S.plan_batches(frames, 4, 0.5, hp) if ragged else [[1], [0, 3], [2]]
        for wav, group in zip(rec.calls, groups):
            for row, idx in enumerate(group):
                S.write_wav(str(tmp_path / "ref.wav"), wav[row, :frames[idx] * hp.hop_size], hp.sample_rate)
                assert (out / (names[idx] + ".wav")).read_bytes() == (tmp_path / "ref.wav").read_bytes(), (ragged, names[idx])


def test_synthesize_out_rate_with_window(cli_case, tmp_path):
    """--window without --device_rng: the clips longer than the window (a, c, d) are resampled too - header rate and frame count."""
    from tf_flowavenet_amd import synthesize as S
    root, hp, model = cli_case
    S.synthesize(_args(root, tmp_path / "w", out_rate=8000, window=1024, ragged=True, max_pad_frac=0.5), hp, model)
    up, down = R.ratio(hp.sample_rate, 8000)
    for name, frames in CLIPS:
        rate, pcm = _read(tmp_path / "w" / (name + ".wav"))
        assert rate == 8000 and len(pcm) == R.n_out(frames * hp.hop_size, up, down) and np.abs(pcm).max() > 0


def test_out_rate_with_device_rng_is_a_parser_error(cli_case, tmp_path, capsys):
    from tf_flowavenet_amd import synthesize as S
    root, _, _ = cli_case
    with pytest.raises(SystemExit) as e:
        S.main(["--saved_dir", str(root / "ckpt"), "--mels_dir", str(root / "mels"), "--output_dir", str(tmp_path / "o"),
                "--device_rng", "--out_rate", "8000"])
    assert e.value.code == 2 and "--out_rate" in capsys.readouterr().err
    assert not (tmp_path / "o").exists()
