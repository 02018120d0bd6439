"""The ``train.py`` loop around the recorded step, host ``Dataset`` against ``--device_corpus`` (one GPU):

    python tools/bench_train_loop.py --out profiles/device_corpus.json

writes a synthetic preprocessing output - 256 utterances of seeded noise, 60 - 900 frames each - into a temporary directory and
runs the loop body of ``train.train`` (draw, ``accumulate`` K - 1 times, ``step``, ``float(loss)``) on the full model at B = 8
clips of T = 6 400 samples.  Legs: batches from the host ``Dataset`` (memory-mapped ``.npy``, crops copied into fresh arrays,
uploaded from pageable memory; with ``--ragged`` a blocking lengths copy) or from ``DeviceCorpus.draw``; plain or ragged; K = 1
or 4 micro-batches per update.  The legs of a mode share one trainer - the recordings are keyed by what is passed, not by where
it came from - and alternate round by round; a round is ``--steps`` updates of wall clock.  Medians over ``--rounds`` rounds,
one JSON line, also written to ``--out``.  The draw alone (``fwn_corpus_draw``: the gather and the counter's advance) is timed
by device events beside it, and so is the host ``Dataset.next_train`` alone by wall clock."""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch


def write_corpus(root, hp, n_utt, lo, hi, seed=0):
    """``train.txt`` + ``audios/`` + ``mels/`` of seeded noise, ``n_utt`` utterances of lo .. hi frames -> the path of train.txt."""
    rng = np.random.default_rng(seed)
    for sub in ("audios", "mels"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    lines = []
    for k in range(n_utt):
        frames = int(rng.integers(lo, hi + 1))
        audio = (0.3 * rng.standard_normal(frames * hp.hop_size)).astype(np.float32)
        mel = rng.standard_normal((frames, hp.num_mels)).astype(np.float32)
        np.save(os.path.join(root, "audios", "u%03d-audio.npy" % k), audio)
        np.save(os.path.join(root, "mels", "u%03d-mel.npy" % k), mel)
        lines.append("u%03d-audio.npy|u%03d-mel.npy|%d|0|noise" % (k, k, len(audio)))
    path = os.path.join(root, "train.txt")
    with open(path, "wt", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="updates per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=6400)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--accum", default="1,4", help="micro-batches per update, comma-separated")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.corpus import DeviceCorpus
    from tf_flowavenet_amd.train import Dataset
    from tf_flowavenet_amd.training import Trainer
    torch.cuda.set_device(0)
    hp = default_hparams().replace(max_time_steps=a.samples, batch_size=a.batch)
    ks = [int(k) for k in a.accum.split(",")]
    with tempfile.TemporaryDirectory() as root:
        path = write_corpus(root, hp, a.utterances, 60, 900)
        sources, trainers = {}, {}
        for ragged in (False, True):
            ds = Dataset(path, hp, seed=3, ragged=ragged)
            sources[ragged] = {"host": ds, "device": DeviceCorpus(ds, hp, seed=3)}
            tr = trainers[ragged] = Trainer(hp, W.synthetic_params(hp, 1234))
            mels, audios = ds.next_full() if ragged else ds.next_train()
            tr.ddi(audios, mels)

        def update(ragged, where, k):
            """One update as ``train.train`` runs it, down to the loss read that ends it."""
            tr, src = trainers[ragged], sources[ragged][where]
            for micro in range(k):
                run = tr.step if micro == k - 1 else tr.accumulate
                if where == "device":
                    audios, mels, lens = src.draw(a.batch)
                    out = run(audios, mels, lengths=lens)
                elif ragged:
                    mels, audios, lens = src.next_train()
                    out = run(audios, mels, lengths=lens)
                else:
                    mels, audios = src.next_train()
                    out = run(audios, mels)
            return float(out[0])

        legs = [(ragged, where, k) for ragged in (False, True) for k in ks for where in ("host", "device")]
        name = lambda leg: "%s_%s_k%d" % (leg[1], "ragged" if leg[0] else "plain", leg[2])
        for leg in legs:                        # eager, record, replay - of every kind of micro-batch this K has
            for _ in range(3):
                loss = update(*leg)
        torch.cuda.synchronize()
        ms = {name(leg): [] for leg in legs}
        for _ in range(a.rounds):
            for leg in legs:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = update(*leg)
                torch.cuda.synchronize()
                ms[name(leg)].append((time.perf_counter() - t0) / a.steps * 1e3)
        # the two ways of making a batch, alone
        alone = {}
        for ragged in (False, True):
            tag = "ragged" if ragged else "plain"
            corpus, ds = sources[ragged]["device"], sources[ragged]["host"]
            times = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    corpus.draw(a.batch)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) / 20)
            alone["device_draw_%s_ms" % tag] = float(np.median(times))
            times = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                for _ in range(20):
                    ds.next_train()
                times.append((time.perf_counter() - t0) / 20 * 1e3)
            alone["host_next_train_%s_ms" % tag] = float(np.median(times))
        lay = sources[True]["device"].layout
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rec = {"metric": "train.py loop, ms per update (draw + K micro-batches + loss read, one GPU), n_block=8 bf16", "unit": "ms per update",
               "config": {"clips": a.batch, "samples_per_clip": a.samples, "utterances": lay.n_utt, "frames": [60, 900],
                          "corpus_bytes": lay.nbytes, "updates_per_round": a.steps, "rounds": a.rounds, "micro_batches": ks},
               "ms_per_update": med,
               "device_over_host": {name(l)[len("device_"):]: med[name(l)] / med[name((l[0], "host", l[2]))] for l in legs if l[1] == "device"},
               "rounds_ms": ms, "batch_alone": alone, "recorded": {("ragged" if r else "plain"): bool(t.graph) for r, t in trainers.items()},
               "loss_finite": bool(np.isfinite(loss))}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
