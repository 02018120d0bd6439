"""``synthesize`` CLI - same flags and file contract as the reference's synthesize.py:51-63:

    python -m tf_flowavenet_amd.synthesize --saved_dir logs/pretrained/ --mels_dir mels/ --output_dir output/

``mels_dir/*.npy`` float32 [F, num_mels] in [0,1]  ->  ``output_dir/<name>.wav`` (16-bit mono PCM at
``hparams.sample_rate``).  Differences: the checkpoint is this package's own format (``*.npz`` /
``*.safetensors`` holding the parameter names of ``weights.param_shapes``, or the reference's own variable
names ``vocoder/FloWaveNet/...:0`` as dumped from a TF checkpoint - ``weights.from_reference_names``; the TF
tensor-bundle format itself is out of scope), the wav writer is the stdlib ``wave`` module (librosa is not a dependency), ``z`` is
seedable (``--seed``; TF's Philox stream cannot be reproduced), and mels of equal length are
batched into one launch.  ``--ragged`` batches mels of *similar* length too (``plan_batches``; ``FloWaveNet.reverse(...,
lengths=)`` gives every clip what it gives alone), and draws each clip's ``z`` from a generator of its own, so a clip's
audio does not depend on the batch it lands in.  ``--device_rng`` (opt-in) keeps the arithmetic on the device
(``FloWaveNet.synthesize``): z comes from a Philox4x32-10 stream keyed by (``--seed``, the clip's index in sorted file-name order) -
a stream of this package's own - with or without ``--ragged``, only the mel goes up and only 16-bit PCM comes down.
``--window SAMPLES`` (opt-in) synthesizes every clip longer than that window by window (``windowing.plan_windows``: each window
with the network's receptive field of real context on both sides, so the seams are exact) - no clip is too long for one call
any more - and writes its wav core by core; the other clips take the paths above.  ``--out_rate HZ`` (opt-in) resamples the
float audio on the device before it is written (``resample.Resampler``: a clip's true samples, ``frames * hop`` of them, not its
padding -> ``ceil(frames * hop * HZ / sample_rate)`` samples, ``write_wav``'s arithmetic, ``HZ`` in the header) on the default
path, with ``--ragged`` and with ``--window``; with ``--device_rng`` - which holds 16-bit PCM, not float audio - it is an error.
``--denoise STRENGTH`` (opt-in) subtracts the model's bias spectrum from every clip on the device (``denoise.Denoiser``: STFT,
soft threshold of the magnitudes by ``STRENGTH`` times the spectrum of what the model synthesizes from nothing, inverse STFT) -
a clip's true samples, before ``--out_rate`` resamples them; with ``--device_rng`` the float waveform stays on the device and
still only int16 comes down; with ``--window`` the stitched clip is denoised whole.
``--wavs_dir DIR`` (opt-in, instead of ``--mels_dir``) is copy-synthesis: every ``DIR/*.wav`` (any PCM rate: ``load_wav``'s reader
and resampler) goes through ``preprocessing.MelFrontEnd`` in ragged batches of ``--batch``, normalised as ``preprocess``
normalises, and its mel enters the paths above as the ``.npy`` of the same name would; the mel comes down to the host and goes
up again with its batch - keeping it on the device between front-end and model is the cut not made.
"""
from __future__ import annotations

import argparse
import glob
import os
import wave

import numpy as np


def load_checkpoint(saved_dir):
    """Latest readable ``*.npz`` / ``*.safetensors`` in ``saved_dir`` -> dict name -> ndarray.  ``...ckpt-<step>.npz``
    files (train.py's) are ordered by step number, anything else by modification time; a file that cannot be read
    (e.g. truncated by a crash) is skipped with a message."""
    import re
    files = glob.glob(os.path.join(saved_dir, "*.npz")) + glob.glob(os.path.join(saved_dir, "*.safetensors"))
    if not files:
        raise FileNotFoundError("no *.npz / *.safetensors checkpoint in %r" % saved_dir)

    def order(path):
        m = re.search(r"ckpt-(\d+)\.npz$", path)
        return (1, int(m.group(1)), 0.0) if m else (0, 0, os.path.getmtime(path))

    from .weights import from_reference_names
    last_error = None
    for path in sorted(files, key=order, reverse=True):
        try:
            if path.endswith(".npz"):
                with np.load(path) as f:
                    raw = {k: f[k] for k in f.files}
            else:
                from safetensors.numpy import load_file
                raw = load_file(path)
        except Exception as e:
            print("Skipping unreadable checkpoint {} ({}: {})".format(path, type(e).__name__, e))
            last_error = e
            continue
        print("Loading checkpoint {}".format(path))
        return from_reference_names(raw)
    raise FileNotFoundError("no readable checkpoint in %r (last error: %s)" % (saved_dir, last_error))


def max_clips_per_call(hparams, t):
    """How many clips of t samples one ``reverse`` call may take: every activation buffer is addressed with 32-bit
    offsets below 2 GiB (csrc/api.hip check_model: n_layer * (B T / 2) * 512 and B * T * num_mels bytes)."""
    lim = min(((1 << 31) - 1) // (hparams.n_layer * 256), ((1 << 31) - 1) // hparams.num_mels)
    return int((lim - 1) // t)


def _aligned_frames(frames, hparams):
    """frames rounded up so that frames * hop divides by 2^n_block (model.py:226)."""
    align = max(1, (1 << hparams.n_block) // int(np.gcd(1 << hparams.n_block, hparams.hop_size)))
    return int(frames) + (-int(frames)) % align


def plan_batches(frame_counts, batch, max_pad_frac, hparams):
    """Which clips share a ragged ``reverse`` call: a list of groups of indices into ``frame_counts`` (mel frames per clip).

    The clips are sorted by length (ties in index order) and taken greedily: a clip joins the open group unless the group
    already holds ``batch`` clips, or ``max_clips_per_call`` at the group's new length would be exceeded, or the padding
    (the samples of the group's ``B * T`` that belong to no clip; T = the longest clip, each clip first rounded up to the
    model's alignment) would exceed ``max_pad_frac`` of ``B * T``.  Padded rows cost what real rows cost, so
    ``max_pad_frac`` trades launches saved against samples wasted: a policy knob, not a correctness one - 0 groups clips
    of equal length only (the grouping without ``--ragged``), the CLI's default is 0.25.  Pure host code."""
    hop = hparams.hop_size
    t_of = [_aligned_frames(f, hparams) * hop for f in frame_counts]
    groups, cur, cur_sum = [], [], 0
    for k in sorted(range(len(t_of)), key=lambda k: (t_of[k], frame_counts[k], k)):
        t = t_of[k]                                  # ascending: the newcomer sets the group's T
        per_call = max_clips_per_call(hparams, t)
        if per_call < 1:
            raise ValueError("an utterance of %d samples exceeds what one call can address (%d samples): split the mel"
                             % (t, max_clips_per_call(hparams, 1)))
        n = len(cur) + 1
        if cur and (n > int(batch) or n > per_call or n * t - (cur_sum + t) > max_pad_frac * n * t):
            groups.append(cur)
            cur, cur_sum = [], 0
        cur.append(k)
        cur_sum += t
    if cur:
        groups.append(cur)
    return groups


def write_wav(path, audio, sample_rate):
    pcm = np.clip(np.asarray(audio, dtype=np.float64), -1.0, 1.0)
    pcm = (pcm * 32767.0).round().astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(pcm.tobytes())


def write_wav_pcm(path, pcm, sample_rate):
    """``write_wav`` for audio that already is 16-bit PCM (``FloWaveNet.synthesize``): the int16 samples go to the file as they are."""
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


class _Output:
    """Where the float paths write their wavs.  Without ``--out_rate``: ``write_wav`` of the clip's true samples at
    ``hparams.sample_rate``, as ever.  With it: the true samples (``lengths``; not a clip's padding) are resampled on the
    device (``resample.Resampler``), ``n_out(length)`` samples per clip come down, and ``write_wav`` writes them with ``HZ`` in
    the header."""

    def __init__(self, args, hparams, denoiser=None):
        self.dir, self.rate, self.resampler, self.denoiser = args.output_dir, int(hparams.sample_rate), None, denoiser
        out_rate = getattr(args, "out_rate", None)
        if out_rate is not None:
            if int(out_rate) < 1:
                raise ValueError("--out_rate must be a positive rate in Hz, got %r" % (out_rate,))
            from .resample import Resampler
            self.rate, self.resampler = int(out_rate), Resampler(hparams.sample_rate, out_rate)

    def path(self, name):
        return os.path.join(self.dir, name[:-4] + ".wav")

    def write(self, names, wav, lengths):
        """``wav``: device float32 [B, T]; clip b is ``names[b]`` with ``lengths[b]`` true samples."""
        if self.denoiser is not None:                # --denoise: at the model's rate, the true samples only
            wav = self.denoiser(wav, lengths=lengths)
        if self.resampler is not None:
            wav = self.resampler(wav, lengths=lengths)
            lengths = [self.resampler.out_length(n) for n in lengths]
        wav = wav.cpu().numpy()
        for n, w, length in zip(names, wav, lengths):
            write_wav(self.path(n), w[:length], self.rate)


def _denoiser(args, model):
    """``--denoise STRENGTH`` -> the model's ``Denoiser`` (its bias is computed here, once per run); None without the flag."""
    strength = getattr(args, "denoise", None)
    if strength is None:
        return None
    from .denoise import Denoiser
    return Denoiser(model, strength=strength)


def mels_from_wavs(wavs_dir, hparams, batch):
    """``--wavs_dir``: every ``*.wav`` in sorted order -> (names, name -> mel float32 [F, num_mels]), ``batch`` files per
    ``MelFrontEnd`` call (any PCM rate: resampled on the device; peak-normalised as ``preprocess`` normalises)."""
    from .preprocessing import MelFrontEnd, load_wavs
    names = sorted(f for f in os.listdir(wavs_dir) if f.endswith(".wav"))
    front, resamplers, mels = MelFrontEnd(hparams), {}, {}
    for i in range(0, len(names), batch):
        group = names[i:i + batch]
        x, lengths = load_wavs([os.path.join(wavs_dir, n) for n in group], hparams.sample_rate, resamplers)
        _, mel, peak = front(x, lengths=lengths, audio=False)
        mel, peak = mel.cpu().numpy(), peak.cpu().numpy()
        for row, n in enumerate(group):
            if not peak[row] > 0.0:
                raise ValueError("%s: silent clip: normalisation divides by max|wav|" % os.path.join(wavs_dir, n))
            mels[n] = mel[row, :1 + lengths[row] // hparams.hop_size].copy()
    return names, mels


def synthesize(args, hparams, model=None):
    import torch
    from .model import FloWaveNet
    if getattr(args, "out_rate", None) is not None and getattr(args, "device_rng", False):
        raise ValueError("--out_rate applies to the float paths: it cannot be combined with --device_rng")
    if model is None:
        model = FloWaveNet(hparams).load_params(load_checkpoint(args.saved_dir))
    denoiser = _denoiser(args, model)
    os.makedirs(args.output_dir, exist_ok=True)
    if getattr(args, "wavs_dir", None) is not None:
        names, mels = mels_from_wavs(args.wavs_dir, hparams, int(args.batch))
    else:
        names = sorted(f for f in os.listdir(args.mels_dir) if f.endswith(".npy"))
        mels = {n: np.load(os.path.join(args.mels_dir, n)).astype(np.float32) for n in names}
    done = set()                                     # --window: the clips longer than it, written window by window
    if getattr(args, "window", None) is not None:
        done = _synthesize_windowed(args, hparams, model, names, mels, window_samples(args.window, hparams), denoiser)
    if getattr(args, "device_rng", False):
        return _synthesize_device(args, hparams, model, names, mels, done, denoiser)
    if getattr(args, "ragged", False):
        return _synthesize_ragged(args, hparams, model, names, mels, done, denoiser)
    by_len = {}
    for n in names:
        if n not in done:
            by_len.setdefault(mels[n].shape[0], []).append(n)
    gen = torch.Generator(device="cpu").manual_seed(int(args.seed))
    out = _Output(args, hparams, denoiser)
    hop = hparams.hop_size
    align = max(1, (1 << hparams.n_block) // np.gcd(1 << hparams.n_block, hop))
    for frames, group in sorted(by_len.items()):
        pad = (-frames) % align                      # T must divide by 2^n_block (model.py:226)
        t = (frames + pad) * hop
        per_call = min(int(args.batch), max_clips_per_call(hparams, t))      # long utterances: fewer clips per launch
        if per_call < 1:
            raise ValueError("an utterance of %d samples exceeds what one call can address (%d samples): split the mel"
                             % (t, max_clips_per_call(hparams, 1)))
        for i in range(0, len(group), per_call):
            chunk = group[i:i + per_call]
            c = np.stack([np.pad(mels[n], ((0, pad), (0, 0)), mode="edge") for n in chunk])
            z = torch.randn(len(chunk), t, 1, generator=gen) * hparams.temp     # synthesize.py:14
            wav = model.reverse(z.cuda(), torch.from_numpy(c).cuda()).squeeze(-1)
            out.write(chunk, wav, [frames * hop] * len(chunk))
    return names


def _synthesize_ragged(args, hparams, model, names, mels, done=(), denoiser=None):
    """``--ragged``: clips of similar length share a call (``plan_batches``).  Each clip is edge-padded to the model's
    alignment as without the flag - that is its ``length`` - and zero-padded from there to the group's T; clip k (in sorted
    file-name order) draws its z from ``torch.Generator().manual_seed(seed + k)``.  ``done``: names ``--window`` has written."""
    import torch
    hop = hparams.hop_size
    frames = [mels[n].shape[0] for n in names]
    keep = [k for k, n in enumerate(names) if n not in done]
    out = _Output(args, hparams, denoiser)
    for group in plan_batches([frames[k] for k in keep], int(args.batch), float(getattr(args, "max_pad_frac", 0.25)), hparams):
        group = [keep[j] for j in group]
        own = [_aligned_frames(frames[k], hparams) for k in group]        # frames of each clip after its own edge padding
        top = max(own)
        c = np.zeros((len(group), top, hparams.num_mels), dtype=np.float32)
        z = torch.zeros(len(group), top * hop, 1)
        for row, (k, f) in enumerate(zip(group, own)):
            c[row, :f] = np.pad(mels[names[k]], ((0, f - frames[k]), (0, 0)), mode="edge")
            gen = torch.Generator(device="cpu").manual_seed(int(args.seed) + k)
            z[row, :f * hop] = torch.randn(f * hop, 1, generator=gen) * hparams.temp
        wav = model.reverse(z.cuda(), torch.from_numpy(c).cuda(), lengths=[f * hop for f in own]).squeeze(-1)
        out.write([names[k] for k in group], wav, [frames[k] * hop for k in group])
    return names


def device_batches(frame_counts, args, hparams):
    """The calls of ``--device_rng``: a list of groups of indices into ``frame_counts``.  With ``--ragged`` ``plan_batches``;
    without it clips of equal length only, in ascending length, ``--batch`` (or what one call can address) at a time - the
    grouping of the host path.  Pure host code."""
    if getattr(args, "ragged", False):
        return plan_batches(frame_counts, int(args.batch), float(getattr(args, "max_pad_frac", 0.25)), hparams)
    by_len = {}
    for k, f in enumerate(frame_counts):
        by_len.setdefault(f, []).append(k)
    groups = []
    for f, ks in sorted(by_len.items()):
        t = _aligned_frames(f, hparams) * hparams.hop_size
        per_call = min(int(args.batch), max_clips_per_call(hparams, t))
        if per_call < 1:
            raise ValueError("an utterance of %d samples exceeds what one call can address (%d samples): split the mel"
                             % (t, max_clips_per_call(hparams, 1)))
        groups += [ks[i:i + per_call] for i in range(0, len(ks), per_call)]
    return groups


def synthesize_device(model, hparams, mel_list, groups, seed, ragged, emit, denoiser=None):
    """The device path over ``groups`` (lists of indices into ``mel_list``, arrays [F, num_mels]): per group one upload of the
    padded mels, one ``FloWaveNet.synthesize`` - clip k draws the z of (seed, clip id k) - and one non-blocking copy of the int16
    result into one of two pinned host buffers.  ``emit(k, pcm)`` gets clip k's samples (a view of the pinned buffer, valid
    during the call) once the group's copy has landed - and that is after the NEXT group has been enqueued, so the device
    works while the host writes files.  One event orders it: recorded behind each copy and waited for before that copy's buffer
    is read; the buffers alternate, so the copy enqueued next never lands in the one being read.  ``denoiser`` (``--denoise``):
    the call also returns its float waveform, which stays on the device; the denoiser turns each clip's true samples into the
    int16 that comes down, on the same stream."""
    import torch
    hop = hparams.hop_size
    frames = [int(m.shape[0]) for m in mel_list]
    pinned = [None, None]
    done = torch.cuda.Event()
    pending = None                                   # (group, T, buffer) of the call whose copy `done` marks

    def flush():
        done.synchronize()
        group, t, buf = pending
        host = buf[:len(group) * t].numpy().reshape(len(group), t)
        for row, k in enumerate(group):
            emit(k, host[row, :frames[k] * hop])

    for n, group in enumerate(groups):
        own = [_aligned_frames(frames[k], hparams) for k in group]        # frames of each clip after its own edge padding
        top = max(own)
        c = np.zeros((len(group), top, hparams.num_mels), dtype=np.float32)
        for row, (k, f) in enumerate(zip(group, own)):
            c[row, :f] = np.pad(mel_list[k], ((0, f - frames[k]), (0, 0)), mode="edge")
        if not ragged and min(own) != top:
            raise ValueError("clips of different lengths share a call only with ragged=True")
        if denoiser is None:
            pcm = model.synthesize(torch.from_numpy(c).cuda(), seed, clip_ids=list(group),
                                   lengths=[f * hop for f in own] if ragged else None)
        else:
            wav = model.synthesize(torch.from_numpy(c).cuda(), seed, clip_ids=list(group),
                                   lengths=[f * hop for f in own] if ragged else None, return_wav=True)[1]
            pcm = denoiser(wav[:, :, 0], lengths=[frames[k] * hop for k in group], pcm=True)
        if pending is not None:
            flush()                                  # the previous group: its buffer is the OTHER one
        need = len(group) * top * hop
        if pinned[n & 1] is None or pinned[n & 1].numel() < need:
            pinned[n & 1] = torch.empty(need, dtype=torch.int16).pin_memory()
        pinned[n & 1][:need].copy_(pcm.reshape(-1), non_blocking=True)
        done.record()
        pending = (group, top * hop, pinned[n & 1])
    if pending is not None:
        flush()


def _synthesize_device(args, hparams, model, names, mels, done=(), denoiser=None):
    """``--device_rng``: clip k (in sorted file-name order) has clip id k under ``--seed``, with and without ``--ragged`` - the
    same seed gives a clip the same z in either mode; the padding rules are those of the host paths.  ``done``: names
    ``--window`` has written (they keep their index: the other clips' ids do not move)."""
    mel_list = [mels[n] for n in names]
    keep = [k for k, n in enumerate(names) if n not in done]
    groups = [[keep[j] for j in g] for g in device_batches([mel_list[k].shape[0] for k in keep], args, hparams)]

    def emit(k, pcm):
        write_wav_pcm(os.path.join(args.output_dir, names[k][:-4] + ".wav"), pcm, hparams.sample_rate)

    synthesize_device(model, hparams, mel_list, groups, int(args.seed), bool(getattr(args, "ragged", False)), emit, denoiser)
    return names


def window_samples(window, hparams):
    """``--window SAMPLES`` rounded up to a multiple of lcm(hop_size, 2^n_block), the unit every window edge sits on."""
    from .windowing import round_up_to_unit
    if int(window) < 1:
        raise ValueError("--window must be a positive number of samples, got %r" % (window,))
    return round_up_to_unit(window, hparams)


def _synthesize_windowed(args, hparams, model, names, mels, window, denoiser=None):
    """``--window``: every clip longer than ``window`` samples (after its edge padding), one at a time, through
    ``FloWaveNet.synthesize_windowed`` (``--device_rng``: clip id = the clip's index in sorted file-name order, as without the
    flag) or ``FloWaveNet.reverse_windowed`` (z drawn on the host from ``torch.Generator().manual_seed(seed + index)``, the
    per-clip generator of ``--ragged``), ``--batch`` windows per call.  The result stays on the device and comes down core by
    core into ``wave``'s incremental ``writeframes``: the host never holds more than one window of audio, and no clip is too
    long for one call.  ``denoiser`` (``--denoise``): the stitched clip is whole on the device - its true samples are denoised
    whole there (with ``--device_rng`` from the float waveform to int16), before ``--out_rate`` resamples them.  -> the set of
    names written."""
    import torch
    from .windowing import plan_windows
    hop = hparams.hop_size
    device_rng = bool(getattr(args, "device_rng", False))
    out = _Output(args, hparams)                     # --out_rate (never with --device_rng): the whole clip is resampled on
    done = set()                                     # the device, and comes down in pieces of the window's size
    for k, name in enumerate(names):
        frames = int(mels[name].shape[0])
        own = _aligned_frames(frames, hparams)
        if own * hop <= window:
            continue
        c = torch.from_numpy(np.pad(mels[name], ((0, own - frames), (0, 0)), mode="edge")[None]).cuda()
        if device_rng:
            if denoiser is None:
                audio = model.synthesize_windowed(c, int(args.seed), clip_ids=[k], window=window, batch=int(args.batch))[0]
            else:
                wav = model.synthesize_windowed(c, int(args.seed), clip_ids=[k], window=window, batch=int(args.batch), return_wav=True)[1]
                audio = denoiser(wav[0, :frames * hop, 0], pcm=True)
        else:
            gen = torch.Generator(device="cpu").manual_seed(int(args.seed) + k)
            z = torch.randn(1, own * hop, 1, generator=gen) * hparams.temp
            audio = model.reverse_windowed(z.cuda(), c, window, batch=int(args.batch))[0, :, 0]
            if denoiser is not None:
                audio = denoiser(audio[:frames * hop])
        pieces = [(a, min(b, frames * hop)) for _, _, a, b in plan_windows(own * hop, window, hparams)]
        if out.resampler is not None:
            audio = out.resampler(audio[:frames * hop].contiguous())
            pieces = [(a, min(a + window, len(audio))) for a in range(0, len(audio), window)]
        with wave.open(out.path(name), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(out.rate)
            for a, b in pieces:
                part = audio[a:b].cpu().numpy()
                if not device_rng:                   # write_wav's arithmetic
                    part = (np.clip(part.astype(np.float64), -1.0, 1.0) * 32767.0).round()
                w.writeframes(np.ascontiguousarray(part, dtype="<i2").tobytes())
        done.add(name)
    return done


class _Given(argparse.Action):
    """Stores the value and notes that the option was given explicitly (``--wavs_dir`` refuses an explicit ``--mels_dir``)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace._given = getattr(namespace, "_given", ()) + (self.dest,)


def main(argv=None):
    from .hparams import hparams
    parser = argparse.ArgumentParser()
    parser.add_argument("--saved_dir", default="logs/pretrained/", help="Folder with model checkpoint")
    parser.add_argument("--mels_dir", default="mels/", action=_Given, help="folder to contain mels to synthesize audio from using the model")
    parser.add_argument("--output_dir", default="output/", help="folder to contain synthesized audio files")
    parser.add_argument("--seed", type=int, default=hparams.tf_random_seed, help="seed of the latent z")
    parser.add_argument("--batch", type=int, default=8, help="mels per launch (of equal length; of similar length with --ragged)")
    parser.add_argument("--ragged", action="store_true",
                        help="batch mels of different lengths into one launch; z is then drawn per clip from seed + index")
    parser.add_argument("--max_pad_frac", type=float, default=0.25,
                        help="with --ragged: the largest share of a launch's samples that may be padding (policy: launches "
                             "saved against samples wasted)")
    parser.add_argument("--device_rng", action="store_true",
                        help="draw z on the device (Philox4x32-10 keyed by --seed and the clip's index: not the default z) and "
                             "bring 16-bit PCM back instead of fp32")
    # absent from the namespace unless given: without the flag the arguments are what they were
    parser.add_argument("--window", type=int, default=argparse.SUPPRESS, metavar="SAMPLES",
                        help="synthesize clips longer than SAMPLES (rounded up to lcm(hop_size, 2^n_block)) window by window, each "
                             "with the network's receptive field of real context on both sides: no length limit, same audio")
    parser.add_argument("--out_rate", type=int, default=argparse.SUPPRESS, metavar="HZ",
                        help="resample the audio on the device to HZ before it is written (default: hparams.sample_rate, no "
                             "resampling); the float paths only - not with --device_rng")
    from .denoise import strength_arg
    parser.add_argument("--denoise", type=strength_arg, default=argparse.SUPPRESS, metavar="STRENGTH",
                        help="subtract STRENGTH times the model's bias spectrum (what it synthesizes from nothing) from every "
                             "clip's STFT magnitudes on the device; a finite number >= 0, typically 0.01 - 0.1")
    parser.add_argument("--wavs_dir", default=argparse.SUPPRESS, metavar="DIR",
                        help="copy-synthesis: take the mels from DIR/*.wav (any PCM rate; normalised as preprocess normalises) "
                             "through the device front-end instead of --mels_dir/*.npy")
    args = parser.parse_args(argv)
    given = vars(args).pop("_given", ())             # not part of the namespace the paths see
    if getattr(args, "wavs_dir", None) is not None and "mels_dir" in given:
        parser.error("--wavs_dir cannot be combined with --mels_dir: the mels come from one or the other")
    if getattr(args, "out_rate", None) is not None:
        if args.device_rng:
            parser.error("--out_rate cannot be combined with --device_rng (the device path holds 16-bit PCM, not float audio)")
        if args.out_rate < 1:
            parser.error("--out_rate must be a positive rate in Hz")
    synthesize(args, hparams)


if __name__ == "__main__":
    main()
