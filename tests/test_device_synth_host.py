"""Host checks of the device-side synthesis path: the Philox4x32-10 restatement the GPU tests compare against
(tests/philox_ref.py) against known answers and its own moments, the PCM wav writer, and the CLI flag.  No GPU."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402

from tf_flowavenet_amd import synthesize as S  # noqa: E402


def test_philox_block_function_known_answers():
    """counter, key -> output.  The first and the third are the published Random123 vectors (zeros; the digits of pi)."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("%08x" % int(v[0]) for v in P.philox4x32_10(counter, key))
        assert got == want, (counter, key, got)
    # vectorised over the first counter word: lane k is the scalar call with counter (k, 0, 0, 0)
    many = P.philox4x32_10((np.arange(5, dtype=np.uint64), 0, 0, 0), (75, 0))
    for k in range(5):
        one = P.philox4x32_10((k, 0, 0, 0), (75, 0))
        assert [int(v[k]) for v in many] == [int(v[0]) for v in one]


def test_latent_stream_known_answer():
    want = [0.928611, 0.021610, -0.386214, -0.745989, 0.894460, -0.466219, 0.164161, -0.352001]
    got = P.latent_normal(75, 0, 8, 0.7)
    assert np.abs(got - np.asarray(want)).max() <= 1e-6, got          # six printed decimals
    # a prefix is a prefix, whatever n; the seed is taken mod 2^64; the clip id and the high key word are live
    assert np.array_equal(P.latent_normal(75, 0, 5, 0.7), got[:5])
    assert np.array_equal(P.latent_normal(75 + (1 << 64), 0, 8, 0.7), got)
    assert np.array_equal(P.latent_normal(75 - (1 << 64), 0, 8, 0.7), got)
    assert not np.array_equal(P.latent_normal(75, 1, 8, 0.7), got)
    assert not np.array_equal(P.latent_normal(75 + (1 << 32), 0, 8, 0.7), got)
    z = P.latent_batch(75, [0, 3], 12, 0.7, lengths=[12, 5])
    assert np.array_equal(z[0, :8], got) and not z[1, 5:].any() and np.array_equal(z[1, :5], P.latent_normal(75, 3, 5, 0.7))


def test_latent_stream_moments():
    """2^20 samples at temp 1: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N) (five standard errors of either estimate),
    max |z| <= sqrt(-2 ln 2^-24) (the smallest u1 the 24-bit mapping produces)."""
    n = 1 << 20
    for seed, clip in ((75, 0), (75, 3), ((1 << 32) + 75, (1 << 32) - 1)):
        z = P.latent_normal(seed, clip, n)
        mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
        print("seed %d clip %d: mean %.5f var-1 %.5f max %.4f" % (seed, clip, mean, var - 1.0, top))
        assert abs(mean) <= 5.0 / np.sqrt(n), (seed, clip, mean)
        assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n), (seed, clip, var)
        assert top <= np.sqrt(-2.0 * np.log(2.0 ** -24)) + 1e-12, (seed, clip, top)


def test_write_wav_pcm_writes_the_bytes_of_write_wav(tmp_path):
    rng = np.random.default_rng(3)
    audio = np.concatenate([0.5 * rng.standard_normal(4096), [1.0, -1.0, 1.5, -1.5, 0.0, 0.5 / 32767.0, 1.5 / 32767.0, -2.5 / 32767.0]]).astype(np.float32)
    S.write_wav(str(tmp_path / "a.wav"), audio, 22050)
    S.write_wav_pcm(str(tmp_path / "b.wav"), P.pcm16(audio), 22050)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    with wave.open(str(tmp_path / "b.wav")) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, audio.size)
    # a strided int16 view (a row of a batch cut to the clip's length) is written as its samples
    block = np.stack([P.pcm16(audio), P.pcm16(-audio)])
    S.write_wav_pcm(str(tmp_path / "c.wav"), block[0, :100], 8000)
    with wave.open(str(tmp_path / "c.wav")) as w:
        assert np.array_equal(np.frombuffer(w.readframes(100), dtype="<i2"), block[0, :100]) and w.getframerate() == 8000


def _parsed(monkeypatch, argv):
    seen = []
    monkeypatch.setattr(S, "synthesize", lambda args, hparams: seen.append(args))
    S.main(argv)
    return vars(seen[0])


def test_cli_flag_parses_and_the_default_namespace_is_unchanged(monkeypatch):
    from tf_flowavenet_amd.hparams import hparams
    base = dict(saved_dir="logs/pretrained/", mels_dir="mels/", output_dir="output/", seed=hparams.tf_random_seed, batch=8,
                ragged=False, max_pad_frac=0.25)
    got = _parsed(monkeypatch, [])
    assert got.pop("device_rng") is False          # opt-in
    assert got == base                             # every flag the CLI had, with the default it had
    assert _parsed(monkeypatch, ["--device_rng"])["device_rng"] is True
    both = _parsed(monkeypatch, ["--device_rng", "--ragged", "--seed", "7", "--batch", "4"])
    assert (both["device_rng"], both["ragged"], both["seed"], both["batch"]) == (True, True, 7, 4)


def test_device_batches_group_like_the_host_paths():
    from tf_flowavenet_amd.hparams import hparams
    frames = [5, 3, 7, 5, 5]
    plain = type("A", (), dict(batch=2, ragged=False))()
    assert S.device_batches(frames, plain, hparams) == [[1], [0, 3], [4], [2]]          # equal lengths only, --batch at a time
    ragged = type("A", (), dict(batch=8, ragged=True, max_pad_frac=0.25))()
    assert S.device_batches(frames, ragged, hparams) == S.plan_batches(frames, 8, 0.25, hparams)
