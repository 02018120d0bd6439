"""GPU tests of the spectral denoiser (csrc/denoise.hip, tf_flowavenet_amd/denoise.py) against its fp64 restatement
(tests/denoise_ref.py; DESIGN.md 6b has the definition and the derivation of the two error bounds asserted here)."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import denoise_ref as R
from conftest import small_hparams
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import weights as W
from tf_flowavenet_amd.denoise import Denoiser
from tf_flowavenet_amd.model import FloWaveNet

pytestmark = pytest.mark.gpu

SHAPES = [(32, 8), (64, 16), (64, 32), (512, 96), (1024, 256)]
U = 2.0 ** -24
GUARD = 64
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _lengths(lib, n_fft, hop):
    """The smallest legal clip, the passthrough, an odd one, and one tile, one tile + 1, three tiles + 1 of the kernel's own."""
    tile = lib.fwn_denoise_tile(n_fft, hop)
    assert tile > 0
    return [n_fft // 2 + 1, n_fft // 2, 7 * hop + 5, tile, tile + 1, 3 * tile + 1]


_CASES = {}


def _case(lib, n_fft, hop):
    """Clips, bias and the fp64 / float32-NumPy results for one shape, computed once and shared (never modified)."""
    key = (n_fft, hop)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n_fft + hop)
        lens = _lengths(lib, n_fft, hop)
        clips = [np.clip(rng.normal(0.0, 0.3, n), -1.0, 1.0).astype(np.float32) for n in lens]
        bias = (rng.uniform(0.0, 1.0, n_fft // 2 + 1) * 0.1 * np.sqrt(n_fft)).astype(np.float32)     # around the bins' own size
        ref = {s: [R.denoise(c.astype(np.float64), bias.astype(np.float64), float(np.float32(s)), n_fft, hop) for c in clips]
               for s in (0.5, 0.0)}
        f32 = {s: [R.denoise(c, bias, s, n_fft, hop) for c in clips] for s in (0.5, 0.0)}
        terms = [R.sample_bound_terms(c, n_fft, hop) if len(c) >= n_fft // 2 + 1 else None for c in clips]
        _CASES[key] = (lens, clips, bias, ref, f32, terms)
    return _CASES[key]


def _sample_bound(terms, ref, n_fft):
    S, env, _ = terms
    return (16 * np.log2(n_fft) + 16) * U * S / env + 4 * U * np.abs(ref)


def _clip_bound(terms, ref, n_fft):
    _, env, V = terms
    return (16 * np.log2(n_fft) + 6) * U * np.sqrt((V ** 2).sum() / env.min()) + 4 * U * np.linalg.norm(ref)


def _run(lib, clips, bias, s, n_fft, hop, pcm=False, len_host=None, len_dev=True, lens_override=None):
    """One fwn_denoise call over a ragged batch, inside guard bands: NaN (float) / 12345 (PCM) prefilled outputs, a row of
    sentinels above and below and GUARD elements beside every row, NaN in the input past every clip's end.  -> [B, T] ndarray."""
    B = len(clips)
    T = max(max(len(c) for c in clips), 1) if len_host is None else len_host
    stride = T + GUARD
    x = np.full((B, stride), np.nan, dtype=np.float32)
    for b, c in enumerate(clips):
        x[b, :len(c)] = c
    fill = 12345 if pcm else np.nan
    out = torch.full((B + 2, stride), fill, dtype=torch.int16 if pcm else torch.float32, device=DEV)
    xd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(np.asarray(bias, dtype=np.float32)).to(DEV)
    lens = [len(c) for c in clips] if lens_override is None else lens_override
    ld = torch.tensor(lens, dtype=torch.int64, device=DEV) if len_dev else None
    o = out[1:].data_ptr()
    rc = lib.fwn_denoise(xd.data_ptr(), B, stride, ld.data_ptr() if len_dev else None, T, bd.data_ptr(), float(s), n_fft, hop,
                         None if pcm else o, stride, o if pcm else None, stride, None, 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "fwn_denoise")
    got = out.cpu().numpy()
    untouched = (lambda a: np.isnan(a).all()) if not pcm else (lambda a: (a == 12345).all())
    assert untouched(got[0]) and untouched(got[-1]) and untouched(got[1:-1, T:]), "something outside [0, T) of a row was written"
    return got[1:-1, :T]


def test_refusals_return_before_any_launch(lib):
    """The pointers below are not device memory: a call that got as far as a launch would fault."""
    P = 1 << 20

    def dn(x=P, B=1, xs=1000, lens=None, n=1000, bias=P, s=0.5, n_fft=64, hop=16, y=P + (1 << 16), ys=1000, pcm=None, ps=1000, ws=None, wb=0):
        rc = lib.fwn_denoise(x, B, xs, lens, n, bias, s, n_fft, hop, y, ys, pcm, ps, ws, wb, None)
        if rc != 0:
            assert b"fwn_denoise" in lib.fwn_last_error()
        return rc

    for bad in (0, 16, 48, 1000, 8192, -64):
        assert dn(n_fft=bad) == -1 and b"power of two" in lib.fwn_last_error(), bad
    for bad in (0, -1, 33, 64):
        assert dn(hop=bad) == -1 and b"hop" in lib.fwn_last_error(), bad
    assert dn(x=None) == -1 and dn(bias=None) == -1 and dn(y=None, pcm=None) == -1
    assert dn(x=P + 2) == -1 and dn(bias=P + 1) == -1 and dn(y=P + (1 << 16) + 2) == -1 and dn(y=None, pcm=P + (1 << 16) + 1) == -1
    assert dn(lens=P + 4) == -1
    assert dn(B=0) == -1 and dn(B=65536) == -1 and dn(n=0) == -1 and dn(n=-5) == -1
    assert dn(xs=999) == -1 and dn(ys=999) == -1 and dn(y=None, pcm=P + (1 << 16), ps=999) == -1
    assert dn(B=65535, xs=1 << 60) == -1 and dn(ys=(1 << 44) + 1) == -1                 # B * stride * 4 would leave int64
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert dn(s=bad) == -1 and b"strength" in lib.fwn_last_error(), bad
    assert dn(ws=None, wb=16) == -1 and b"workspace" in lib.fwn_last_error()
    assert dn(y=P) == -1 and dn(y=P + 400) == -1 and b"overlaps" in lib.fwn_last_error()
    assert lib.fwn_denoise_workspace_bytes(4, 100000, 1024, 256) == 0
    assert lib.fwn_denoise_tile(1024, 256) > 0 and lib.fwn_denoise_tile(1000, 256) == -1 and lib.fwn_denoise_tile(64, 33) == -1

    def mm(x=P, B=1, xs=1000, n=1000, n_fft=64, hop=16, out=P + (1 << 16)):
        rc = lib.fwn_stft_mean_mag(x, B, xs, n, n_fft, hop, out, None)
        if rc != 0:
            assert b"fwn_stft_mean_mag" in lib.fwn_last_error()
        return rc

    assert mm(n_fft=96) == -1 and mm(hop=0) == -1 and mm(hop=33) == -1
    assert mm(x=None) == -1 and mm(out=None) == -1 and mm(x=P + 1) == -1 and mm(out=P + 2) == -1
    assert mm(B=0) == -1 and mm(B=65536) == -1 and mm(xs=999) == -1 and mm(n=0) == -1
    assert mm(n=63) == -1 and b"no interior frame" in lib.fwn_last_error()
    assert mm(n=70, hop=24) == -1 and b"no interior frame" in lib.fwn_last_error()      # frame 2 ends at 80
    assert mm(B=65535, xs=1 << 21, n=1 << 21, hop=1) == -1                              # more frames than one workgroup is given


_WORST = {}


@pytest.mark.parametrize("n_fft,hop", SHAPES)
@pytest.mark.parametrize("s", [0.5, 0.0])
def test_kernel_matches_restatement_within_both_bounds(lib, n_fft, hop, s):
    lens, clips, bias, ref, f32, terms = _case(lib, n_fft, hop)
    got = _run(lib, clips, bias, s, n_fft, hop)
    for b, n in enumerate(lens):
        y = got[b, :n]
        assert np.all(got[b, n:] == 0.0) and not np.signbit(got[b, n:]).any()
        if n < n_fft // 2 + 1:
            assert np.array_equal(y.view(np.uint32), clips[b].view(np.uint32))           # passthrough, bit for bit
            continue
        r = ref[s][b]
        err = np.abs(y - r)
        per_sample, per_clip = _sample_bound(terms[b], r, n_fft), _clip_bound(terms[b], r, n_fft)
        e2, f2 = np.linalg.norm(y - r), np.linalg.norm(f32[s][b].astype(np.float64) - r)
        mult = e2 / f2 if f2 > 0 else 0.0
        _WORST[(n_fft, hop)] = max(_WORST.get((n_fft, hop), 0.0), mult)
        print("n_fft %d hop %d s %.1f N %d: max err / per-sample bound %.4f, clip err / clip bound %.4f, float32 NumPy at %.4f; "
              "kernel error = %.2f x float32 NumPy's" % (n_fft, hop, s, n, (err / per_sample).max(), e2 / per_clip, f2 / per_clip, mult))
        assert np.all(err <= per_sample), (n, int(np.argmax(err / per_sample)), float((err / per_sample).max()))
        assert e2 <= per_clip, (n, e2, per_clip)
        if s == 0.0:
            assert np.abs(y - clips[b]).max() <= per_sample.max()
    print("worst kernel error as a multiple of float32 NumPy's, n_fft %d hop %d: %.2f" % (n_fft, hop, _WORST[(n_fft, hop)]))


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (1024, 256)])
def test_past_a_clips_length_is_plus_zero_and_pcm_zero_and_len_host_alone_works(lib, n_fft, hop):
    lens, clips, bias, ref, _, terms = _case(lib, n_fft, hop)
    T = max(lens) + 77
    y = _run(lib, clips, bias, 0.5, n_fft, hop, len_host=T)
    p = _run(lib, clips, bias, 0.5, n_fft, hop, pcm=True, len_host=T)
    for b, n in enumerate(lens):
        assert np.all(y[b, n:].view(np.uint32) == 0) and np.all(p[b, n:] == 0)
    # no len_dev: every row is len_host long
    n = lens[2]
    one = _run(lib, [clips[2]], bias, 0.5, n_fft, hop, len_dev=False)
    assert np.array_equal(one[0].view(np.uint32), y[2, :n].view(np.uint32))


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (512, 96), (1024, 256)])
def test_ragged_batch_gives_each_clip_the_bits_it_gets_alone(lib, n_fft, hop):
    lens, clips, bias, _, _, _ = _case(lib, n_fft, hop)
    pick = [5, 1, 2, 4]                                       # three tiles + 1, the passthrough, an odd one, one tile + 1
    batch = _run(lib, [clips[k] for k in pick], bias, 0.5, n_fft, hop)
    for row, k in enumerate(pick):
        alone = _run(lib, [clips[k]], bias, 0.5, n_fft, hop)
        assert np.array_equal(alone[0].view(np.uint32), batch[row, :lens[k]].view(np.uint32)), (n_fft, hop, lens[k])
    # a device length above len_host is clamped to it; a negative one to 0
    n = lens[2]
    over = _run(lib, [clips[2], clips[2]], bias, 0.5, n_fft, hop, lens_override=[n + 1000, -3])
    assert np.array_equal(over[0].view(np.uint32), batch[2, :n].view(np.uint32)) and np.all(over[1].view(np.uint32) == 0)


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (1024, 256)])
def test_pcm_is_fwn_pcm16_of_the_float_result_and_within_one_lsb_of_the_restatement(lib, n_fft, hop):
    lens, clips, bias, ref, _, terms = _case(lib, n_fft, hop)
    y = _run(lib, clips, bias, 0.5, n_fft, hop)
    p = _run(lib, clips, bias, 0.5, n_fft, hop, pcm=True)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    want = torch.empty(y.shape, dtype=torch.int16, device=DEV)
    _lib.check(lib.fwn_pcm16(yd.data_ptr(), want.data_ptr(), y.shape[0], y.shape[1], None, torch.cuda.current_stream().cuda_stream), "fwn_pcm16")
    assert np.array_equal(p, want.cpu().numpy())
    for b, n in enumerate(lens):
        if n < n_fft // 2 + 1:
            continue
        _one_lsb_rule(p[b, :n], ref[0.5][b], terms[b], n_fft, "N %d" % n)


def _one_lsb_rule(pcm, r64, terms, n_fft, what):
    """Against write_wav's arithmetic on the fp64 restatement: at most 1 LSB off, and only where the fp64 value lies within the
    per-sample bound x 32767 of a rounding boundary."""
    scaled = np.clip(r64, -1.0, 1.0) * 32767.0
    diff = np.abs(pcm.astype(np.int64) - scaled.round().astype(np.int64))
    assert diff.max() <= 1, (what, int(diff.max()))
    moved = diff > 0
    to_half = np.abs(np.abs(scaled - np.floor(scaled)) - 0.5)
    assert np.all(to_half[moved] <= _sample_bound(terms, r64, n_fft)[moved] * 32767.0), what
    print("%s: %d of %d samples one LSB off" % (what, int(moved.sum()), len(pcm)))


def test_denoiser_module_takes_lists_tensors_and_one_clip(lib):
    n_fft, hop = 64, 16
    lens, clips, bias, ref, _, terms = _case(lib, n_fft, hop)
    d = Denoiser(bias=bias, n_fft=n_fft, hop=hop, strength=0.5)
    T = max(lens)
    x = torch.zeros(len(clips), T, device=DEV)
    for b, c in enumerate(clips):
        x[b, :len(c)] = torch.from_numpy(c)
    want = _run(lib, clips, bias, 0.5, n_fft, hop)
    for given in (lens, torch.tensor(lens, dtype=torch.int64, device=DEV)):
        y = d(x, lengths=given)
        assert y.dtype == torch.float32 and y.shape == x.shape and np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    p = d(x, lengths=lens, pcm=True)
    assert p.dtype == torch.int16 and np.array_equal(p.cpu().numpy(), _run(lib, clips, bias, 0.5, n_fft, hop, pcm=True))
    one = d(x[2, :lens[2]])
    assert one.shape == (lens[2],) and np.array_equal(one.cpu().numpy().view(np.uint32), want[2, :lens[2]].view(np.uint32))
    zero = d(x[2, :lens[2]], strength=0.0)
    assert np.abs(zero.cpu().numpy() - clips[2]).max() <= _sample_bound(terms[2], clips[2].astype(np.float64), n_fft).max()
    with pytest.raises(ValueError):
        d(x, lengths=lens[:-1])
    with pytest.raises(TypeError):
        d(x.double())


def test_bias_from_a_tiny_model():
    hp = small_hparams(n_fft=64)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 3, actnorm="random"))
    d = Denoiser(model)
    assert (d.n_fft, d.hop, d.nb) == (64, 16, 33) and d.bias.shape == (33,) and d.bias.dtype == torch.float32
    audio = d.bias_audio.cpu().numpy()
    assert audio.shape == (1, 64 * 16)
    b = d.bias.cpu().numpy()
    assert np.isfinite(b).all() and (b >= 0.0).all() and b.max() > 0.0
    want = R.mean_mag(audio, 64, 16)
    lo, hi = R.interior(audio.shape[1], 64, 16)
    v = np.sqrt((R.frames(audio[0].astype(np.float64), 64, 16)[lo:hi + 1] ** 2).sum(axis=1)).mean()
    bound = (8 * 6 + 4) * U * np.sqrt(64.0) * v
    err = np.abs(b - want).max()
    print("bias of the tiny model: max |kernel - restatement| = %.3e, bound %.3e (%d interior frames)" % (err, bound, hi - lo + 1))
    assert err <= bound
    again = Denoiser(model)
    assert np.array_equal(again.bias.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert Denoiser(model, bias_frames=10).bias_audio.shape == (1, 160)


def test_element_offsets_past_2_to_the_31(lib):
    """One [1, N] row of 2^31 + 5000 samples (8.6 GB in, 8.6 GB out): 4096 samples at the start, across element 2^31 and at the
    end against the restatement of the span around them (an output depends on the samples within n_fft of it only)."""
    n_fft, hop, span = 1024, 256, 4096
    N = (1 << 31) + 5000
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * 4 * N:                                       # the largest row this device's memory allows
        N = int(free // 12)
        print("only %d bytes of device memory free: the row is %d samples, below 2^31" % (free, N))
    assert N > 8 * span
    x = torch.empty(N, dtype=torch.float32, device=DEV)
    step = 1 << 28
    gen = torch.Generator(device=DEV).manual_seed(5)
    for a in range(0, N, step):                                # N(0, 0.3^2) clipped to [-1, 1], drawn in pieces
        x[a:a + step].normal_(0.0, 0.3, generator=gen).clamp_(-1.0, 1.0)
    bias = (np.random.default_rng(9).uniform(0.0, 1.0, n_fft // 2 + 1) * 0.1 * np.sqrt(n_fft)).astype(np.float32)
    y = Denoiser(bias=bias, n_fft=n_fft, hop=hop, strength=0.5)(x)
    assert y.shape == (N,)
    for a in (0, min(1 << 31, N // 2) - span // 2, N - span):
        lo = max(0, (a - 2 * n_fft) // hop * hop)              # a multiple of hop: the sub-clip's frames are the clip's
        hi = min(N, a + span + 2 * n_fft)
        sub = x[lo:hi].cpu().numpy()
        ref = R.denoise(sub.astype(np.float64), bias.astype(np.float64), 0.5, n_fft, hop)
        terms = R.sample_bound_terms(sub, n_fft, hop)
        got = y[a:a + span].cpu().numpy()
        err = np.abs(got - ref[a - lo:a - lo + span])
        bound = _sample_bound(terms, ref, n_fft)[a - lo:a - lo + span]
        print("samples [%d, %d): max err / bound %.4f" % (a, a + span, (err / bound).max()))
        assert np.all(err <= bound), a
        assert np.abs(got).max() > 0.0


# ---- the CLI at a tiny model ----

CLIPS = [("a", 40), ("b", 23), ("c", 40), ("d", 61)]       # mel frames; hop 16: 640, 368, 640 and 976 samples
STRENGTH = 0.1


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    root = tmp_path_factory.mktemp("cli_denoise")
    hp = small_hparams(n_fft=64)
    params = W.synthetic_params(hp, 2, actnorm="random")
    (root / "mels").mkdir()
    rng = np.random.default_rng(0)
    for name, frames in CLIPS:
        np.save(root / "mels" / (name + ".npy"), rng.random((frames, hp.num_mels), dtype=np.float32))
    model = FloWaveNet(hp).load_params(params)
    return root, hp, model, Denoiser(model, strength=STRENGTH).bias.cpu().numpy()


class _Recorder:
    """The model the CLI drives, keeping the float audio of every call: the CLI's own z, the CLI's own batches."""

    def __init__(self, model):
        self._model, self.float_audio = model, {}

    def __getattr__(self, name):
        return getattr(self._model, name)

    def _keep(self, wav):
        self.float_audio[len(self.float_audio)] = wav.reshape(wav.shape[0], -1).cpu().numpy().copy()

    def reverse(self, z, c, *a, **kw):
        wav = self._model.reverse(z, c, *a, **kw)
        if bool((z != 0).any()):                               # (not the denoiser's own call for the bias)
            self._keep(wav)
        return wav

    def reverse_windowed(self, *a, **kw):
        wav = self._model.reverse_windowed(*a, **kw)
        self._keep(wav)
        return wav

    def synthesize(self, *a, **kw):
        kw["return_wav"] = True
        pcm, wav = self._model.synthesize(*a, **kw)
        self._keep(wav)
        return pcm, wav

    def synthesize_windowed(self, *a, **kw):
        kw["return_wav"] = True
        pcm, wav = self._model.synthesize_windowed(*a, **kw)
        self._keep(wav)
        return pcm, wav


class _Plain(_Recorder):
    """The same recorder for a run WITHOUT the flag: the CLI asks for PCM alone and gets PCM alone."""

    def synthesize(self, *a, **kw):
        assert "return_wav" not in kw
        return _Recorder.synthesize(self, *a, **kw)[0]

    def synthesize_windowed(self, *a, **kw):
        assert "return_wav" not in kw
        return _Recorder.synthesize_windowed(self, *a, **kw)[0]


def _args(root, out, **kw):
    base = dict(mels_dir=str(root / "mels"), output_dir=str(out), seed=75, batch=4)
    base.update(kw)
    return type("A", (), base)()


def _read(path):
    with wave.open(str(path)) as w:
        assert (w.getnchannels(), w.getsampwidth()) == (1, 2)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


@pytest.mark.parametrize("path", ["default", "ragged", "device_ragged", "window"])
def test_cli_denoise(cli_case, tmp_path, path):
    """--denoise 0.1: every wav is write_wav of the restatement applied to what the same command without the flag synthesizes
    (under the 1-LSB rule), and without the flag the wavs are write_wav / the PCM of that audio, byte for byte, as before."""
    from tf_flowavenet_amd import synthesize as S
    root, hp, model, bias = cli_case
    extra = {"default": {}, "ragged": dict(ragged=True, max_pad_frac=0.5), "device_ragged": dict(device_rng=True, ragged=True, max_pad_frac=0.5),
             "window": dict(window=800, ragged=True, max_pad_frac=0.5)}[path]
    plain, rec = _Plain(model), _Recorder(model)
    S.synthesize(_args(root, tmp_path / "plain", **extra), hp, plain)
    S.synthesize(_args(root, tmp_path / "dn", denoise=STRENGTH, **extra), hp, rec)
    assert len(plain.float_audio) == len(rec.float_audio) >= 1
    rows = []                                                  # every row of float audio the model returned, in call order
    for k in range(len(rec.float_audio)):
        assert np.array_equal(plain.float_audio[k], rec.float_audio[k])        # the flag changes nothing upstream
        rows += list(rec.float_audio[k])
    hop = hp.hop_size
    for name, frames in CLIPS:
        n = frames * hop
        before, after = _read(tmp_path / "plain" / (name + ".wav")), _read(tmp_path / "dn" / (name + ".wav"))
        assert len(before) == len(after) == n
        # the clip's float audio: the one row whose write_wav / PCM is the file written without the flag
        mine = [r for r in rows if len(r) >= n and np.array_equal(R.pcm16(r[:n]), before)]
        assert mine, name
        x = mine[0][:n]
        S.write_wav(str(tmp_path / "ref.wav"), x, hp.sample_rate)
        assert (tmp_path / "plain" / (name + ".wav")).read_bytes() == (tmp_path / "ref.wav").read_bytes()
        r64 = R.denoise(x.astype(np.float64), bias.astype(np.float64), float(np.float32(STRENGTH)), 64, hop)
        _one_lsb_rule(after, r64, R.sample_bound_terms(x, 64, hop), 64, "%s %s" % (path, name))
        print("%s %s: the denoiser moved %d of %d samples" % (path, name, int((before != after).sum()), n))
    if path == "window":
        assert any(a.shape == (1, 61 * hop) for a in rec.float_audio.values())       # clip d went window by window
