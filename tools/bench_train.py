"""Training-step benchmark (BASELINE configs[2]: data-parallel training, batch 8 per GPU, 6400-sample
crops, full n_block=8 n_flow=6 model).  One process per GPU:

    python tools/bench_train.py --steps 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        tools/bench_train.py --gpus N --steps 10

Each step = gradients of -(log_p + logdet) on this rank's batch (HIP stage kernels), RCCL all-reduce
of the flat fp32 gradient, global-norm clip, Adam.  Prints one JSON line (whole-job samples/s).

    python tools/bench_train.py --ragged --out profiles/ragged_training.json

times three steps on one GPU, alternating them round by round in one process: the plain step, the ragged step
(``Trainer.step(x, c, lengths=)``) with every length = T, and the ragged step with lengths spread over 1024 .. T; one JSON
line with the per-round figures and their medians (also written to ``--out``).

    python tools/bench_train.py --accum 2,4,8 --out profiles/accum_training.json

times, the same way, the plain step against one optimiser update over K micro-batches (``Trainer.accumulate`` K - 1 times, then
``Trainer.step``) for every K given: ms per update, ms per micro-batch, samples/s; and the fold kernel alone over the whole flat
gradient buffer beside ``adam_clip_kernel``, in bytes/s from device events."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch


def ragged_leg(a):
    """Plain | ragged with full lengths | ragged with spread lengths, B = a.batch clips of a.samples samples, one trainer each on
    the same initial weights; rounds of a.steps steps alternate between the three (a round ends in a synchronise)."""
    import math
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.training import Trainer
    torch.cuda.set_device(0)
    hp = default_hparams()
    unit = math.lcm(hp.hop_size, 1 << hp.n_block)
    inp = W.synthetic_inputs(hp, a.batch, a.samples)
    x, c = torch.from_numpy(inp["x"]).reshape(a.batch, a.samples).cuda(), torch.from_numpy(inp["c"]).cuda()
    lo = min(max(unit, 1024 // unit * unit), a.samples)
    spread = [int(round((lo + (a.samples - lo) * k / max(1, a.batch - 1)) / unit)) * unit for k in range(a.batch)]
    legs = {"plain": None, "ragged_full": [a.samples] * a.batch, "ragged_spread": spread}
    trainers = {}
    for name in legs:
        tr = trainers[name] = Trainer(hp, W.synthetic_params(hp, 1234))
        tr.ddi(x, c)
        for _ in range(max(a.warmup, 3)):       # eager, record, replay
            tr.step(x, c, lengths=legs[name]) if legs[name] is not None else tr.step(x, c)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, lens in legs.items():
            tr = trainers[name]
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = tr.step(x, c, lengths=lens) if lens is not None else tr.step(x, c)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    rec = {"metric": "training step, ms (forward + backward + clip/Adam, one GPU), n_block=8 bf16", "unit": "ms per step",
           "config": {"clips": a.batch, "samples_per_clip": a.samples, "spread_lengths": spread, "steps_per_round": a.steps,
                      "rounds": a.rounds},
           "ms_per_step": {k: float(np.median(v)) for k, v in ms.items()}, "rounds_ms": ms,
           "recorded": {k: bool(trainers[k].graph) for k in legs}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def accum_leg(a):
    """Plain step | one update over K micro-batches for every K of a.accum, B = a.batch clips of a.samples samples, one trainer
    each on the same initial weights; rounds of a.steps updates alternate between the legs (a round ends in a synchronise).
    Then the fold alone - ``fwn_grad_accumulate(g, acc, g)`` over the whole flat buffer, 12 bytes per element - beside
    ``adam_clip_kernel`` (``fwn_clip_adam``, 28 bytes per element) on buffers of the same length, both timed by device events."""
    from tf_flowavenet_amd import _lib
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.training import Trainer
    torch.cuda.set_device(0)
    hp = default_hparams()
    inp = W.synthetic_inputs(hp, a.batch, a.samples)
    x, c = torch.from_numpy(inp["x"]).reshape(a.batch, a.samples).cuda(), torch.from_numpy(inp["c"]).cuda()
    ks = [int(k) for k in a.accum.split(",")]
    if any(k < 2 for k in ks):
        raise SystemExit("--accum takes K >= 2 (the plain step is always a leg)")
    legs = {"plain": 1}
    legs.update({"accum_%d" % k: k for k in ks})

    def update(tr, k):
        for _ in range(k - 1):
            tr.accumulate(x, c)
        return tr.step(x, c)

    trainers = {}
    for name, k in legs.items():
        tr = trainers[name] = Trainer(hp, W.synthetic_params(hp, 1234))
        tr.ddi(x, c)
        for _ in range(max(a.warmup, 3)):       # eager, record, replay - of every kind of micro-batch this K has
            update(tr, k)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, k in legs.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                update(trainers[name], k)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    # the fold and the optimiser kernel alone, on the K = max trainer's buffers (its accumulator exists); Adam on scratch
    # copies so that no trainer's state is touched
    lib, opt = _lib.load(), trainers["accum_%d" % max(ks)].opt
    n, st = opt.g.numel(), torch.cuda.current_stream().cuda_stream
    w2, m2, v2, one = opt.w.clone(), torch.zeros_like(opt.w), torch.zeros_like(opt.w), torch.ones(1, device="cuda")
    g, acc = opt.g, opt.acc
    kernels = {
        "fold": (12, lambda: lib.fwn_grad_accumulate(g.data_ptr(), acc.data_ptr(), g.data_ptr(), n, st)),
        "first_store": (8, lambda: lib.fwn_grad_accumulate(acc.data_ptr(), None, g.data_ptr(), n, st)),
        "adam_clip": (28, lambda: lib.fwn_clip_adam(w2.data_ptr(), g.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, one.data_ptr(), 1.0, 1.0,
                                                    1e-3, 1, 0.9, 0.999, 1e-8, st)),
    }
    alone = {}
    for name, (nbytes, launch) in kernels.items():
        for _ in range(3):
            _lib.check(launch(), name)
        times = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                _lib.check(launch(), name)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 10)
        t = float(np.median(times))
        alone[name] = {"ms": t, "bytes_per_element": nbytes, "bytes_per_s": nbytes * n / (t * 1e-3)}
    rec = {"metric": "training update over K micro-batches, ms (one GPU), n_block=8 bf16", "unit": "ms per update",
           "config": {"clips": a.batch, "samples_per_clip": a.samples, "updates_per_round": a.steps, "rounds": a.rounds, "flat_elements": n},
           "ms_per_update": med,
           "ms_per_micro_batch": {name: med[name] / k for name, k in legs.items()},
           "samples_per_s": {name: a.batch * a.samples * k / (med[name] * 1e-3) for name, k in legs.items()},
           "rounds_ms": ms, "kernels_alone": alone,
           "fold_over_adam_bytes_per_s": alone["fold"]["bytes_per_s"] / alone["adam_clip"]["bytes_per_s"],
           "recorded": {name: bool(trainers[name].graph) for name in legs}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=6400)
    ap.add_argument("--ragged", action="store_true", help="one GPU: plain step | ragged step, full lengths | lengths 1024 .. samples")
    ap.add_argument("--rounds", type=int, default=5, help="--ragged / --accum: rounds of --steps steps (updates) per leg, alternating")
    ap.add_argument("--accum", default="", help="one GPU: plain step | one update over K micro-batches, for every K of this comma-separated list")
    ap.add_argument("--out", default="", help="--ragged / --accum: also write the JSON line to this file")
    a = ap.parse_args()
    if a.ragged:
        return ragged_leg(a)
    if a.accum:
        return accum_leg(a)
    import torch.distributed as dist
    from tf_flowavenet_amd.hparams import default_hparams
    from tf_flowavenet_amd import weights as W
    from tf_flowavenet_amd.training import Trainer
    world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    # FWN_BENCH_SHARE_GPU=1: plumbing check on a one-GPU box (every rank on cuda:0, exchanges over gloo)
    share = os.environ.get("FWN_BENCH_SHARE_GPU") == "1"
    torch.cuda.set_device(0 if share else int(os.environ.get("LOCAL_RANK", 0)))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if share else "nccl")
    hp = default_hparams()
    inp = W.synthetic_inputs(hp, a.batch, a.samples)
    x = torch.from_numpy(np.roll(inp["x"], 997 * rank, axis=1)).reshape(a.batch, a.samples).cuda()
    c = torch.from_numpy(np.roll(inp["c"], rank, axis=1)).cuda()
    tr = Trainer(hp, W.synthetic_params(hp, 1234))
    tr.ddi(x, c)
    for _ in range(a.warmup):
        tr.step(x, c)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, lp, ld, gn = tr.step(x, c)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        tm = torch.tensor([el], device="cuda", dtype=torch.float64)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        el = float(tm)
    if rank == 0:
        print(json.dumps({"metric": "training audio samples/sec (forward + backward + all-reduce + clip/Adam), n_block=8 bf16",
                          "value": a.batch * a.samples * world * a.steps / el, "unit": "samples/s", "n_gpus": world,
                          "steps": a.steps, "warmup": a.warmup, "ms_per_step": el / a.steps * 1e3,
                          "config": {"workload": "configs[2]: data-parallel training step", "clips_per_gpu": a.batch,
                                     "samples_per_clip": a.samples}, "loss": float(loss), "grad_norm": float(gn)}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
