"""GPU tests of the ragged mel front-end (csrc/melfront.hip) against tests/mel_front_ref.py: the peak and the padded
audio bit for bit, the mel inside the restatement's per-element bound, the locality rule (ragged batch = every clip alone, a
hop-aligned slice = the whole clip), offsets past 2^31, and the three surfaces: preprocess(batch=), synthesize --wavs_dir,
MelStream."""
import os
import wave

import numpy as np
import pytest
import torch

import mel_front_ref as R
from conftest import small_hparams
from tf_flowavenet_amd import _lib
from tf_flowavenet_amd import preprocessing as P
from tf_flowavenet_amd.hparams import default_hparams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 777.0
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


_TABLES = {}


def _tables(hp):
    key = (hp.n_fft, hp.hop_size, hp.num_mels)
    if key not in _TABLES:
        fb = P.mel_filterbank(hp)
        _TABLES[key] = (fb, torch.from_numpy(fb).to(DEV), torch.from_numpy(P.mel_bands(fb)).to(DEV))
    return _TABLES[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(lib, clips, hp, normalize=True, bands=True, audio=True, len_host=None, len_dev=True, x_off=0):
    """fwn_clip_peak + fwn_mel_front over ``clips`` in one ragged batch: NaN behind every clip's end, junk in the peak buffer,
    sentinel guard bands around every output row (checked here).  -> (peak [B], mel [B, F_host, M], audio [B, F_host hop])."""
    B, hop, M = len(clips), hp.hop_size, hp.num_mels
    lens = [len(c) for c in clips]
    L = len_host or max(max(lens), 1)
    F = 1 + L // hop
    xs = L + 3                                                 # odd stride: rows start at every alignment
    host = np.full(x_off + B * xs, np.nan, dtype=np.float32)
    for b, c in enumerate(clips):
        host[x_off + b * xs:x_off + b * xs + len(c)] = c
    x = torch.from_numpy(host).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int64, device=DEV) if len_dev else None
    assert len_dev or all(n == L for n in lens)
    peak = torch.full((B + 2,), 12345.0, device=DEV)
    ms, as_ = F * M + GUARD, F * hop + GUARD
    mel = torch.full((GUARD + B * ms,), SENTINEL, device=DEV)
    aud = torch.full((GUARD + B * as_,), SENTINEL, device=DEV)
    _, fb, bd = _tables(hp)
    xp = x.data_ptr() + 4 * x_off
    _lib.check(lib.fwn_clip_peak(xp, B, xs, None if ld is None else ld.data_ptr(), L, peak.data_ptr() + 4, None), "fwn_clip_peak")
    rc = lib.fwn_mel_front(xp, B, xs, None if ld is None else ld.data_ptr(), L, peak.data_ptr() + 4 if normalize else None,
                           float(hp.rescaling_max) if normalize else 1.0, fb.data_ptr(), bd.data_ptr() if bands else None, hp.n_fft, hop, M,
                           float(hp.ref_level_db), float(hp.min_level_db), mel.data_ptr() + 4 * GUARD, ms,
                           aud.data_ptr() + 4 * GUARD if audio else None, as_, None)
    _lib.check(rc, "fwn_mel_front")
    torch.cuda.synchronize()
    peak, mel, aud = peak.cpu().numpy(), mel.cpu().numpy(), aud.cpu().numpy()
    assert peak[0] == 12345.0 and peak[-1] == 12345.0
    assert np.all(mel[:GUARD] == SENTINEL) and np.all(aud[:GUARD] == SENTINEL)
    mel, aud = mel[GUARD:].reshape(B, ms), aud[GUARD:].reshape(B, as_)
    assert np.all(mel[:, F * M:] == SENTINEL) and np.all(aud[:, F * hop:] == SENTINEL)
    if not audio:
        assert np.all(aud == SENTINEL)
    return peak[1:-1], mel[:, :F * M].reshape(B, F, M), aud[:, :F * hop]


def _check_clip(x, hp, pk, mel, aud, what, normalize=True):
    """One clip's row against the restatement: peak and audio bit for bit, +0 behind the clip, the mel inside the bound.
    -> (worst |err| / bound, float32 NumPy's worst on the same input)."""
    hop = hp.hop_size
    a0, m0, p0, xn = R.front(x, hp, normalize)
    f = R.frames_of(len(x), hop)
    assert (np.isnan(pk) and np.isnan(p0)) or _bits(pk) == _bits(p0), (what, pk, p0)
    assert np.array_equal(_bits(aud[:f * hop]), _bits(a0)), what
    assert not _bits(aud[f * hop:]).any() and not _bits(mel[f:]).any(), what
    if len(x) < hp.n_fft // 2 + 1 or (normalize and not p0 > 0.0):
        assert not _bits(mel).any(), what
        return 0.0, 0.0
    fb = _tables(hp)[0]
    bd = R.bound(xn, hp, fb)
    err = np.abs(mel[:f].astype(np.float64) - m0)
    ratio, r32 = float((err / bd).max()), float((np.abs(R.mel32(xn, hp, fb) - m0) / bd).max())
    print("%s: worst |err| / bound %.4f (float32 NumPy %.4f), bound.max() %.2e" % (what, ratio, r32, bd.max()))
    assert np.all(err <= bd), (what, ratio)
    return ratio, r32


# ---- the peak ----

def test_peak_is_numpys_bit_for_bit(lib):
    hp = R.hp_of(64, 16, 8)
    lens = [0, 1, 255, 256, 257, 100003]
    clips = [R.signal(40 + n, n) for n in lens]
    clips[3][17] = -3.5                                        # a negative maximum
    for x_off in (0, 1, 2, 3):
        pk, _, _ = _run(lib, clips, hp, x_off=x_off)
        assert np.array_equal(_bits(pk), _bits([R.peak(c) for c in clips])), x_off
        assert _bits(pk)[0] == 0
    for c in clips[1:]:                                        # alone: B, the row, the stride and len_host do not matter
        assert _bits(_run(lib, [c], hp)[0])[0] == _bits(R.peak(c))
    assert _bits(_run(lib, [clips[5]], hp, len_dev=False)[0])[0] == _bits(R.peak(clips[5]))
    for at in (0, 20000, 100002):                              # a NaN inside shows, in whichever workgroup's part it lies
        bad = [c.copy() for c in clips]
        bad[5][at] = np.nan
        bad[1][0] = np.nan
        pk, mel, aud = _run(lib, bad, hp)
        assert np.isnan(pk[5]) and np.isnan(pk[1]) and np.array_equal(_bits(pk[[0, 2, 3, 4]]), _bits([R.peak(c) for c in clips])[[0, 2, 3, 4]])
        assert not _bits(mel[5]).any() and not _bits(aud[5]).any()
    inf = clips[4].copy()
    inf[100] = -np.inf
    assert _run(lib, [inf], hp)[0][0] == np.inf


# ---- audio and mel against the restatement ----

def _edge_lengths(lib, n_fft, hop):
    g = lib.fwn_mel_front_frames(n_fft, hop)
    assert g >= 1
    return [n_fft // 2 + 1, hop - 1, hop, hop + 1, 3 * g * hop + 1]


@pytest.mark.parametrize("n_fft,hop,n_mels", [(64, 16, 8), (1024, 256, 80)])
def test_audio_is_the_restatements_bits_with_zeros_behind(lib, n_fft, hop, n_mels):
    hp = R.hp_of(n_fft, hop, n_mels)
    clips = [R.signal(60 + i, n) for i, n in enumerate(_edge_lengths(lib, n_fft, hop))]
    pk, mel, aud = _run(lib, clips, hp, len_host=max(len(c) for c in clips) + 5 * hop + 3)
    for b, c in enumerate(clips):
        _check_clip(c, hp, pk[b], mel[b], aud[b], "n_fft %d hop %d N %d" % (n_fft, hop, len(c)))
        pad_l = (R.frames_of(len(c), hop) * hop - len(c)) // 2
        if len(c) >= n_fft // 2 + 1:
            assert aud[b][pad_l] == R.gain(c, pk[b], hp.rescaling_max)[0] and (pad_l == 0 or not aud[b][:pad_l].any())
    pk, mel, aud = _run(lib, clips[:1] + clips[4:], hp, normalize=False)                       # no gain: the samples themselves
    for b, c in enumerate(clips[:1] + clips[4:]):
        _check_clip(c, hp, pk[b], mel[b], aud[b], "n_fft %d hop %d N %d, not normalised" % (n_fft, hop, len(c)), normalize=False)


def _mel_cases(lib):
    cases = list(R.SHAPES)
    for n_fft, hop, n_mels in ((1024, 256, 80), (64, 16, 8), (256, 100, 20)):
        g = lib.fwn_mel_front_frames(n_fft, hop)
        cases += [(n_fft, hop, n_mels, n_fft // 2 + 1), (n_fft, hop, n_mels, 3 * g * hop + 1)]
    return cases


def test_mel_is_inside_the_bound_everywhere(lib):
    worst = (0.0, 0.0, None)
    for n_fft, hop, n_mels, n in _mel_cases(lib):
        hp = R.hp_of(n_fft, hop, n_mels)
        x = R.signal(n + 1, n)
        pk, mel, aud = _run(lib, [x], hp, len_dev=False)
        ratio, r32 = _check_clip(x, hp, pk[0], mel[0], aud[0], "n_fft %d hop %d n_mels %d N %d" % (n_fft, hop, n_mels, n))
        assert 0.0 <= mel.min() and mel.max() <= 1.0 and mel.std() > 0.01
        if ratio > worst[0]:
            worst = (ratio, r32, (n_fft, hop, n_mels, n))
    print("worst |err| / bound over all cases: %.4f at %r (float32 NumPy there: %.4f)" % (worst[0], worst[2], worst[1]))


def test_silent_and_nan_clips_give_zero_rows_and_the_telling_peak(lib):
    hp = R.hp_of(64, 16, 8)
    good = R.signal(1, 500)
    nan = good.copy()
    nan[250] = np.nan
    pk, mel, aud = _run(lib, [np.zeros(500, np.float32), nan, good, -np.zeros(40, np.float32)], hp)
    assert _bits(pk[0]) == 0 and np.isnan(pk[1]) and pk[2] == np.abs(good).max() and _bits(pk[3]) == 0
    for b in (0, 1, 3):
        assert not _bits(mel[b]).any() and not _bits(aud[b]).any()
    _check_clip(good, hp, pk[2], mel[2], aud[2], "the good clip between them")
    assert mel[2].any()


@pytest.mark.parametrize("n_fft,hop,n_mels", [(64, 16, 8), (256, 100, 20), (1024, 256, 80)])
def test_bands_change_no_bit(lib, n_fft, hop, n_mels):
    hp = R.hp_of(n_fft, hop, n_mels)
    clips = [R.signal(70 + i, n) for i, n in enumerate((n_fft // 2 + 1, 7 * hop + 3, 2000))]
    with_bands, dense = _run(lib, clips, hp), _run(lib, clips, hp, bands=False)
    assert np.array_equal(_bits(with_bands[1]), _bits(dense[1])) and with_bands[1].any()
    assert np.array_equal(_bits(with_bands[2]), _bits(dense[2]))


@pytest.mark.parametrize("n_fft,hop,n_mels", [(64, 16, 8), (1024, 256, 80)])
def test_ragged_batch_gives_each_clip_the_bits_it_gets_alone(lib, n_fft, hop, n_mels):
    hp = R.hp_of(n_fft, hop, n_mels)
    g = lib.fwn_mel_front_frames(n_fft, hop)
    lens = [n_fft // 2 + 1, 5 * hop, 2 * g * hop + hop - 1, 3 * g * hop + 1, hop]
    clips = [R.signal(80 + i, n) for i, n in enumerate(lens)]
    pk, mel, aud = _run(lib, clips, hp)
    for b, c in enumerate(clips):
        p1, m1, a1 = _run(lib, [c], hp, len_dev=False)
        f = R.frames_of(len(c), hop)
        assert _bits(pk[b]) == _bits(p1[0])
        assert np.array_equal(_bits(mel[b, :f]), _bits(m1[0])) and not _bits(mel[b, f:]).any()
        assert np.array_equal(_bits(aud[b, :f * hop]), _bits(a1[0])) and not _bits(aud[b, f * hop:]).any()
        assert m1.any() == (len(c) >= n_fft // 2 + 1)


@pytest.mark.parametrize("n_fft,hop,n_mels", [(64, 16, 8), (1024, 256, 80), (256, 100, 20)])
def test_interior_frames_of_a_hop_aligned_slice_are_the_whole_clips(lib, n_fft, hop, n_mels):
    hp = R.hp_of(n_fft, hop, n_mels)
    x = R.signal(90, 40 * hop + 7)
    whole = _run(lib, [x], hp, normalize=False)[1][0]
    for first, frames in ((3, 30), (11, 20)):                  # slices that start on other frames of a workgroup's run
        part = _run(lib, [x[first * hop:(first + frames) * hop]], hp, normalize=False)[1][0]
        need = -(-(n_fft // 2) // hop)                         # slice frames need .. frames - need have their support inside it
        assert frames - 2 * need >= 4 and part.shape[0] == frames + 1
        assert np.array_equal(_bits(part[need:frames - need + 1]), _bits(whole[first + need:first + frames - need + 1]))
        assert not np.array_equal(_bits(part[0]), _bits(whole[first])) and not np.array_equal(_bits(part[frames]), _bits(whole[first + frames]))


# ---- 64-bit addressing ----

def test_row_strides_past_2_to_the_31(lib):
    """B = 2, every stride above 2^31 elements, in buffers that are never filled: row 1 (and row 0) equal the clip alone."""
    hp = R.hp_of(64, 16, 8)
    n, hop, M = 3000, 16, 8
    stride = (1 << 31) + 8
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * 4 * (stride + n) + (1 << 30):
        stride = int((free - (1 << 30)) // 12 - n) // 4 * 4
        print("only %d bytes of device memory free: strides of %d elements, below 2^31" % (free, stride))
    F = 1 + n // hop
    assert stride > F * hop
    x = torch.empty(stride + n, dtype=torch.float32, device=DEV)
    mel = torch.empty(stride + F * M, dtype=torch.float32, device=DEV)
    aud = torch.empty(stride + F * hop, dtype=torch.float32, device=DEV)
    clips = [R.signal(31, n), R.signal(32, n)]
    for b in (0, 1):
        x[b * stride:b * stride + n] = torch.from_numpy(clips[b]).to(DEV)
    peak = torch.empty(2, dtype=torch.float32, device=DEV)
    _, fb, bd = _tables(hp)
    _lib.check(lib.fwn_clip_peak(x.data_ptr(), 2, stride, None, n, peak.data_ptr(), None), "fwn_clip_peak")
    _lib.check(lib.fwn_mel_front(x.data_ptr(), 2, stride, None, n, peak.data_ptr(), float(hp.rescaling_max), fb.data_ptr(), bd.data_ptr(),
                                 64, hop, M, float(hp.ref_level_db), float(hp.min_level_db), mel.data_ptr(), stride, aud.data_ptr(),
                                 stride, None), "fwn_mel_front")
    torch.cuda.synchronize()
    for b in (0, 1):
        p1, m1, a1 = _run(lib, [clips[b]], hp, len_dev=False)
        assert _bits(peak[b].cpu().numpy()) == _bits(p1[0])
        assert np.array_equal(_bits(mel[b * stride:b * stride + F * M].cpu().numpy()), _bits(m1[0]).reshape(-1)) and m1.any()
        assert np.array_equal(_bits(aud[b * stride:b * stride + F * hop].cpu().numpy()), _bits(a1[0]))


def test_element_offsets_past_2_to_the_31(lib):
    """One row of 2^31 + 5000 samples at (4096, 2048, 2 mels): the frames at its start, in its middle and at its end - the row
    ends 5000 samples past element 2^31, so those last frames straddle it - against the restatement of the hop-aligned span
    around them (the locality rule), audio included."""
    n_fft, hop, M = 4096, 2048, 2
    hp = R.hp_of(n_fft, hop, M)
    N = (1 << 31) + 5000
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * 4 * N + (1 << 30):
        N = int((free - (1 << 30)) // 8)
        print("only %d bytes of device memory free: the row is %d samples, below 2^31" % (free, N))
    assert N > 64 * hop
    x = torch.empty(N, dtype=torch.float32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(6)
    for a in range(0, N, 1 << 28):                             # quiet noise, drawn in pieces: at 4096 points N(0, 0.3^2) saturates the mel at 1
        x[a:a + (1 << 28)].normal_(0.0, 0.003, generator=gen).clamp_(-1.0, 1.0)
    x[N - 77] = -1.5                                           # the peak: in the last workgroup's part
    audio, mel, peak = P.MelFrontEnd(hp)(x)
    torch.cuda.synchronize()
    F = 1 + N // hop
    assert mel.shape == (1, F, M) and audio.shape == (1, F * hop) and float(peak[0]) == 1.5
    fb = _tables(hp)[0]
    pad_l = (F * hop - N) // 2
    mid = min(1 << 31, N // 2) // hop
    for f0, f1, lo, hi in ((0, 5, 0, 8 * hop), (mid - 3, mid + 4, (mid - 5) * hop, (mid + 6) * hop), (F - 4, F, (F - 7) * hop, N)):
        sub = R.gain(x[lo:hi].cpu().numpy(), np.float32(1.5), hp.rescaling_max)
        ref = R.onp.melspectrogram(sub.astype(np.float64), hp)[f0 - lo // hop:f1 - lo // hop]
        bd = R.bound(sub, hp, fb)[f0 - lo // hop:f1 - lo // hop]
        err = np.abs(mel[0, f0:f1].cpu().numpy().astype(np.float64) - ref)
        print("frames [%d, %d): worst |err| / bound %.4f" % (f0, f1, (err / bd).max()))
        assert np.all(err <= bd) and 0.05 < ref.min() and ref.max() < 0.95 and ref.std() > 0
        got = audio[0, lo + pad_l:hi + pad_l].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(sub))
    assert not audio[0, :pad_l].any() and not audio[0, pad_l + N:].any()


# ---- the surfaces ----

def _write_wav(path, x, rate):
    pcm = (np.clip(x, -1.0, 1.0) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def test_module_takes_lists_tensors_and_one_clip():
    hp = R.hp_of(64, 16, 8)
    front = P.MelFrontEnd(hp)
    clips = [R.signal(1, 700), R.signal(2, 333)]
    x = np.zeros((2, 700), np.float32)
    x[1, 333:] = np.nan
    x[0], x[1, :333] = clips[0], clips[1]
    a, m, p = front(x, lengths=[700, 333])
    a2, m2, p2 = front(torch.from_numpy(x).to(DEV), lengths=torch.tensor([700, 333], device=DEV))
    assert a.shape == (2, 44 * 16) and m.shape == (2, 44, 8) and p.shape == (2,) and a.device.type == "cuda"
    assert torch.equal(a, a2) and torch.equal(m, m2) and torch.equal(p, p2)
    a1, m1, p1 = front(clips[1])
    assert a1.shape == (1, 21 * 16) and torch.equal(m1[0], m[1, :21]) and torch.equal(a1[0], a[1, :21 * 16]) and not m[1, 21:].any()
    assert front(clips[0], audio=False)[0] is None
    with pytest.raises(ValueError):
        front(x, lengths=[1, 2, 3])


def test_preprocess_batch_writes_the_default_paths_files(tmp_path):
    hp = default_hparams()
    book = tmp_path / "in" / "book1"
    os.makedirs(book / "wavs")
    lines = []
    for i, n in enumerate((3000, 4100, 2999, 5121, 3584)):
        _write_wav(book / "wavs" / ("u%d.wav" % i), R.signal(20 + i, n), hp.sample_rate)
        lines.append("u%d|raw %d|text %d" % (i, i, i))
    _write_wav(book / "wavs" / "u5.wav", R.signal(29, 9000), 48000)
    lines.insert(2, "u5|raw 5|text 5")                         # the other rate in the middle of the first batch
    (book / "metadata.csv").write_text("\n".join(lines), encoding="utf-8")
    P.preprocess(str(tmp_path / "in"), str(tmp_path / "one"), hp)
    meta = P.preprocess(str(tmp_path / "in"), str(tmp_path / "four"), hp, batch=4)
    assert len(meta) == 6
    assert (tmp_path / "four" / "train.txt").read_bytes() == (tmp_path / "one" / "train.txt").read_bytes()
    fb = P.mel_filterbank(hp)
    for sub in ("audios", "mels"):
        assert sorted(os.listdir(tmp_path / "four" / sub)) == sorted(os.listdir(tmp_path / "one" / sub)) and len(os.listdir(tmp_path / "one" / sub)) == 6
    order = ["u0", "u1", "u5", "u2", "u3", "u4"]
    for k, name in enumerate(order):
        a_name, m_name = "dataset-audio-%05d.npy" % (k + 1), "dataset-mel-%05d.npy" % (k + 1)
        a0, a1 = np.load(tmp_path / "one" / "audios" / a_name), np.load(tmp_path / "four" / "audios" / a_name)
        m0, m1 = np.load(tmp_path / "one" / "mels" / m_name), np.load(tmp_path / "four" / "mels" / m_name)
        assert a1.dtype == m1.dtype == np.float32 and a1.shape == a0.shape and m1.shape == m0.shape
        wav = P.load_wav(str(book / "wavs" / (name + ".wav")), hp.sample_rate)
        audio, ref, _, xn = R.front(wav, hp)
        if name != "u5":
            assert (tmp_path / "four" / "audios" / a_name).read_bytes() == (tmp_path / "one" / "audios" / a_name).read_bytes()
        assert np.array_equal(_bits(a1), _bits(audio)), name
        err, bd = np.abs(m1.astype(np.float64) - ref), R.bound(xn, hp, fb)
        print("%s: worst |err| / bound %.4f; against the DFT kernel's file %.2e" % (name, (err / bd).max(), np.abs(m1 - m0).max()))
        assert np.all(err <= bd), name
    _write_wav(book / "wavs" / "u3.wav", np.zeros(4000, np.float32), hp.sample_rate)
    with pytest.raises(ValueError, match="u3.wav"):
        P.preprocess(str(tmp_path / "in"), str(tmp_path / "silent"), hp, batch=4)
    for sub, stem in (("audios", "dataset-audio-"), ("mels", "dataset-mel-")):                  # u3 is in the second batch...
        assert sorted(os.listdir(tmp_path / "silent" / sub)) == ["%s%05d.npy" % (stem, k) for k in (1, 2, 3, 4)]
    with pytest.raises(ValueError, match="u3.wav"):
        P.preprocess(str(tmp_path / "in"), str(tmp_path / "silent2"), hp, batch=5)
    assert os.listdir(tmp_path / "silent2" / "mels") == [] and os.listdir(tmp_path / "silent2" / "audios") == []    # ...here in the first


@pytest.mark.parametrize("path", ["default", "ragged"])
def test_synthesize_wavs_dir_equals_mels_dir_of_the_front_ends_mels(tmp_path, path):
    from tf_flowavenet_amd import synthesize as S
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.model import FloWaveNet
    hp = small_hparams(n_fft=64)
    model = FloWaveNet(hp).load_params(W.synthetic_params(hp, 2, actnorm="random"))
    (tmp_path / "wavs").mkdir()
    (tmp_path / "mels").mkdir()
    front = P.MelFrontEnd(hp)
    for name, n, rate in (("a", 640, hp.sample_rate), ("b", 377, hp.sample_rate), ("c", 640, hp.sample_rate), ("d", 2000, 2 * hp.sample_rate),
                          ("e", 990, hp.sample_rate)):
        _write_wav(tmp_path / "wavs" / (name + ".wav"), R.signal(ord(name), n), rate)
        wav = P.load_wav(str(tmp_path / "wavs" / (name + ".wav")), hp.sample_rate)
        np.save(tmp_path / "mels" / (name + ".npy"), front(wav, audio=False)[1][0].cpu().numpy())
    (tmp_path / "wavs" / "notes.txt").write_text("not a wav")
    extra = dict(ragged=True, max_pad_frac=0.5) if path == "ragged" else {}
    for key, out in (("wavs_dir", "from_wavs"), ("mels_dir", "from_mels")):
        args = type("A", (), dict(output_dir=str(tmp_path / out), seed=3, batch=3, **{key: str(tmp_path / key[:4]), **extra}))()
        names = S.synthesize(args, hp, model)
        assert [n[:-4] for n in names] == ["a", "b", "c", "d", "e"]
    for name in "abcde":
        a, b = (tmp_path / "from_wavs" / (name + ".wav")).read_bytes(), (tmp_path / "from_mels" / (name + ".wav")).read_bytes()
        assert a == b and len(a) > 44 + 2 * 16 * 20, name
    assert sorted(os.listdir(tmp_path / "from_wavs")) == ["a.wav", "b.wav", "c.wav", "d.wav", "e.wav"]


@pytest.mark.parametrize("step", [4096, 7777])
def test_melstream_equals_the_one_call(step):
    hp = default_hparams()
    x = R.signal(step, 50000)
    whole = P.MelFrontEnd(hp)(x, normalize=False, audio=False)[1][0]
    s = P.MelStream(hp)
    parts = [s.push(x[a:a + step]) for a in range(0, len(x), step)] + [s.finish()]
    got = torch.cat([p for p in parts if p is not None])
    assert got.shape == whole.shape == (1 + 50000 // hp.hop_size, hp.num_mels)
    assert torch.equal(got, whole) and bool(whole.std() > 0.01)
    half = P.MelStream(hp, gain=0.5)
    got = torch.cat([p for p in [half.push(x[:30000]), half.push(x[30000:]), half.finish()] if p is not None])
    assert torch.equal(got, P.MelFrontEnd(hp)(x * np.float32(0.5), normalize=False, audio=False)[1][0])
