#!/usr/bin/env python
"""Flagship benchmark: motion-RNN data-parallel training throughput on MI355X.

Measures the reference's headline metric (BASELINE.json): whole-node
sequences/second of the motion LSTM (2 layers x 32 hidden, 9 inputs x 128
timesteps, 6 classes, Adam lr 2.5e-3, fp32 -- the reference's precision)
trained with DDP at a FIXED global batch of 1440 (strong scaling: per-rank
batch = 1440 / N, exactly like reference src/motion/trainer/distributed.py:48-49).
Data are synthetic tensors of the UCI-HAR shape ([6912, 128, 9] fp32), weights
random-init (no network: no dataset or checkpoint download).

The headline ``value`` is the reference's own metric: training sequences per
second over whole epochs (6912 sequences / epoch time, reference
src/motion/trainer/base.py:93-96).  The timed region is EXACTLY ``--steps``
steps starting at an epoch boundary, in sampler order -- full batches and the
short last batch of every epoch (1440 x 4 + 1152 at global batch 1440) -- so
the default ``--steps 50`` is 10 whole epochs.  Every timed step is the full
training step of the CLI's ``distributed`` trainer (``Trainer.train_batch``):
device batch gather, fused LSTM forward, fused cross-entropy, fused BPTT
backward, native RCCL all-reduce, fused Adam.  ``--warmup`` untimed steps
first; the timed region is bracketed by a barrier + device synchronize on both
sides; the MAX elapsed time over ranks is reported by rank 0 as ONE JSON line.
A plain run does only that.  ``--full`` adds ``step_seq_per_s``, a second,
full-batch-only measurement (the per-step figure of earlier rounds), in a
timed run of its own.  ``--dump-outputs DIR`` writes what the last timed step
returned and the parameters it left behind as ``DIR/<name>.npy`` (float32), so
that two builds can be compared output for output.

    python bench.py                       # 1 GPU
    python bench.py --full                # ... and the secondary measurement
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \\
        --master-addr 127.0.0.1 --master-port 29500 bench.py --gpus 8
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC = "sequences/sec (whole node) for motion RNN DDP at 1/2/4/8 MI355X; epoch time"
# Reference DDP (MPI) seq/s at global batch 1440, 1/2/4/8 nodes (dedup table)
BASELINE_SEQ_PER_S = {1: 44.8, 2: 85.9, 4: 128.5, 8: 213.3}
EPOCH_SEQUENCES = 6912
DUMP_MAX_BYTES = 64 * 1000 * 1000  # --dump-outputs: all arrays together
DUMP_SAMPLE_SEED = 20240607


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", 1)))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--global-batch", type=int, default=1440)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--epoch-sequences", type=int, default=EPOCH_SEQUENCES,
                    help="training-set size (default: the reference's 6912); e.g. 864 with --global-batch 180 "
                         "rehearses one rank's epoch of the 8-GPU run on one GPU")
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong",
                    help="strong: global batch fixed (reference); weak: --global-batch per GPU")
    ap.add_argument("--trainer", choices=("distributed", "horovod"), default="distributed")
    ap.add_argument("--cell", choices=("lstm", "gru"), default="lstm")
    ap.add_argument("--seed", type=int, default=123456789)
    ap.add_argument("--cuda-graph", action="store_true",
                    help="replay the synced step (fwd/BPTT, RCCL all-reduce, Adam) from a HIP graph")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32",
                    help="bf16: BASELINE config 2 (bf16 inputs/weights, fp32 accumulate)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary full-batch-only measurement (step_seq_per_s, step_ms_full_batch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (its [loss, n, correct] "
                         "statistics) and left behind (every model parameter) as DIR/<name>.npy (rank 0)")
    return ap.parse_args(argv)


def dump_outputs(directory: str, stats, model) -> None:
    """The timed path's results after its last step, one float32 .npy each:
    ``stats`` = that step's [loss, batch size, correct] (what
    ``Trainer.train_batch`` returns) and ``param.<name>`` = every parameter of
    the model the step updated in place.  With the same arguments the data,
    the initial weights and the batch order are the same from run to run.
    At most DUMP_MAX_BYTES in all: of a model larger than that (--hidden in
    the thousands) every array beyond an equal share keeps a fixed, seeded
    sample of its elements (sorted flat indices, the same from run to run)."""
    import numpy as np
    import torch
    os.makedirs(directory, exist_ok=True)
    arrays = {"stats": stats}
    for name, p in model.state_dict().items():
        arrays["param." + name] = p
    share = None
    if sum(t.numel() for t in arrays.values()) * 4 > DUMP_MAX_BYTES:
        share = DUMP_MAX_BYTES // 4 // len(arrays)
    for name, t in arrays.items():
        a = t.detach().to(device="cpu", dtype=torch.float32).contiguous().numpy()
        if share is not None and a.size > share:
            pick = np.random.default_rng(DUMP_SAMPLE_SEED).choice(a.size, size=share, replace=False)
            a = a.reshape(-1)[np.sort(pick)]
        np.save(os.path.join(directory, name + ".npy"), a)


def _max_over_ranks(x: float, dev) -> float:
    """MAX of a host scalar over ranks: on the native RCCL communicator when
    there is one (the gradient path's), else torch.distributed."""
    import torch
    import torch.distributed as dist
    from pytorch_distributed_rnn_amd.parallel.comm import native_world_comm
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return x
    c = native_world_comm()
    if c is not None:
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        c.all_reduce(t, "max")
        c.wait()
        torch.cuda.synchronize(dev)
        return float(t.item())
    t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def main(argv=None):
    args = parse(argv)
    logging.basicConfig(level=logging.WARNING)
    import torch
    import torch.distributed as dist

    from pytorch_distributed_rnn_amd.data.motion import MotionDataset, synthetic_motion
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    from pytorch_distributed_rnn_amd.parallel import env
    from pytorch_distributed_rnn_amd.train.distributed import DDPTrainer, HorovodTrainer

    torch.manual_seed(args.seed)
    info = env.init_distributed()
    world = env.get_world_size()
    rank = env.get_rank()
    if world != args.gpus and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but world size is {world}", file=sys.stderr)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    n_train = max(args.epoch_sequences, args.global_batch * (world if args.scaling == "weak" else 1))
    train_set, _, _ = synthetic_motion(n_train=n_train, n_validation=1, n_test=1,
                                       seq_length=args.seq_len, seed=args.seed)
    model = MotionModel(train_set.num_features, args.hidden, args.layers,
                        len(MotionDataset.LABELS), cell=args.cell,
                        compute_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    cls = DDPTrainer if args.trainer == "distributed" else HorovodTrainer
    trainer = cls(model=model, training_set=train_set, batch_size=args.global_batch,
                  learning_rate=0.0025, weak_scaling=args.scaling == "weak", device=dev,
                  cuda_graph=True if args.cuda_graph else None)
    per_rank = trainer.train_loader.batch_size

    loader = trainer.train_loader
    steps_per_epoch = len(loader)

    def epoch_batches(first_epoch):
        """Sampler epochs first_epoch, first_epoch+1, ...: every batch of each
        epoch in order, the short last one included (the reference's epoch)."""
        epoch = first_epoch
        while True:
            trainer.sampler.set_epoch(epoch)
            yield from loader.batch_indices()
            epoch += 1

    # PDRNN_TRACE=bench: where the wall time of a timed run goes (stderr):
    # host time to the first step's launch, host enqueue time, device time
    # between events bracketing the run, the final synchronize and barrier
    trace = os.environ.get("PDRNN_TRACE") == "bench" and dev.type == "cuda"

    def timed_run(batches, per_step=False):
        env.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        if trace:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            t_first = None
        stats = None
        # one trainer call per epoch's worth of steps (the multi-GPU fused
        # step replays them from one HIP graph, like the CLI's epoch loop)
        if per_step:
            for b in batches:
                stats, _ = trainer.train_batch(loader.make_batch(b))
                if trace and t_first is None:
                    t_first = time.perf_counter() - t0
        for k in range(0, 0 if per_step else len(batches), steps_per_epoch):
            res = trainer.train_batches([loader.make_batch(b) for b in batches[k:k + steps_per_epoch]])
            stats = res[-1][0]
            if trace and t_first is None:
                t_first = time.perf_counter() - t0
        if trace:
            t_enq = time.perf_counter() - t0
            ev[1].record()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t_sync = time.perf_counter() - t0
        env.barrier()
        elapsed = time.perf_counter() - t0
        if trace:
            print(f"[bench trace] steps {len(batches)} wall {elapsed * 1e3:.3f} ms: first epoch enqueued "
                  f"{t_first * 1e3:.3f}, all enqueued {t_enq * 1e3:.3f}, synced {t_sync * 1e3:.3f}; "
                  f"device events {ev[0].elapsed_time(ev[1]):.3f} ms", file=sys.stderr, flush=True)
        return _max_over_ranks(elapsed, dev), stats

    trainer.model.train()
    # one-time device setup (kernel code-object load, workspace sizing): the
    # trainer's gradient-only pre-pass, no parameter update -- the same
    # preparation the CLI runs before its timed epochs
    trainer.prepare()
    warm = epoch_batches(0)
    warm_steps = [next(warm) for _ in range(args.warmup)]
    for k in range(0, len(warm_steps), steps_per_epoch):
        trainer.train_batches([loader.make_batch(b) for b in warm_steps[k:k + steps_per_epoch]])
    # The timed region: EXACTLY --steps training steps starting at an epoch
    # boundary, in the sampler's epoch order (full batches and the short last
    # batch of every epoch).  With --steps a multiple of the steps per epoch it
    # is E whole epochs and value = epoch_sequences * E / time: the reference's
    # metric (6912 / Training Duration, reference src/motion/trainer/base.py:93-96,
    # evaluation/Experiments.ipynb:49).  The host permutations are drawn up
    # front (the CLI trainer prefetches them during the previous epoch); the
    # batch assembly is inside the timed loop.
    stream = epoch_batches(1000)
    timed = [next(stream) for _ in range(args.steps)]
    local_seqs = sum(int(b.numel()) for b in timed)
    elapsed, stats = timed_run(timed)
    seqs = local_seqs * world  # every rank runs the same batch sizes (per-rank batch = global / world)
    value = seqs / elapsed
    ms = elapsed / args.steps * 1e3
    epochs = args.steps / steps_per_epoch
    global_batch = per_rank * world
    base = BASELINE_SEQ_PER_S.get(world)
    # sanity: loss must be finite after training (read before any later step
    # reuses the row of the statistics ring that ``stats`` is a view of)
    loss = float(stats[0])
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, stats, model)
    step_elapsed = step_value = None
    if args.full:
        # secondary: full-batch step throughput (the short last batch skipped),
        # the per-step figure of earlier rounds
        full = []
        stream = epoch_batches(2000)
        while len(full) < args.steps + 3:
            b = next(stream)
            if b.numel() == per_rank:
                full.append(b)
        for b in full[:3]:  # per-step graph capture of the synced step (N > 1) outside the clock
            trainer.train_batch(loader.make_batch(b))
        step_elapsed, _ = timed_run(full[3:], per_step=True)
        step_value = per_rank * world * args.steps / step_elapsed
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "sequences/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": round(value / base, 2) if base else None,
            "dtype": args.dtype,
            "data": "synthetic (UCI-HAR shape [6912,128,9] fp32, random-init weights)",
            "config": {
                "model": f"motion-{args.cell.upper()} {args.layers}x{args.hidden} (9 inputs -> 6 classes)",
                "global_batch": global_batch,
                "seq_len": args.seq_len,
                "parallelism": f"dp{world}",
                "trainer": args.trainer,
                "per_gpu_batch": per_rank,
            },
            "epochs": round(epochs, 4),
            "steps_per_epoch": steps_per_epoch,
            "epoch_time_s": round(elapsed / epochs, 6),
            "epoch_sequences": n_train,
            "timed_sequences": seqs,
            "final_loss": round(loss, 6),
            "baseline_seq_per_s": base,
        }
        if args.full:
            out["step_seq_per_s"] = round(step_value, 2)
            out["step_ms_full_batch"] = round(step_elapsed / args.steps * 1e3, 4)
        print(json.dumps(out), flush=True)
    env.shutdown()


if __name__ == "__main__":
    main()
