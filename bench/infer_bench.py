#!/usr/bin/env python
"""Motion evaluation: the fused inference path against ``model.forward``.

Evaluates the synthetic 6912-sequence set (fp32, 2 x 32 LSTM and GRU) through
``Trainer._evaluate`` in batches of 1440, 691 (the default validation split)
and 180 sequences, and times one ``MotionModel.predict`` call on one sequence
against one ``model.forward`` call (batch 1: latency).  Both paths run in one
process and alternate after a warm-up: ``PDRNN_FUSED_EVAL=0`` (per-batch
``model.forward``, head GEMM, cross-entropy kernel and host read) and the
fused path (train/fused_eval.py: one launch per batch, one host read per
evaluation).  Every timing is ``--repeats`` evaluations back to back and ends
in a device synchronise (for batch 1 each call synchronises: it is a latency).
Prints one JSON line per (cell, batch size): the pairs in ms per evaluation,
both medians and ranges, and whether the fused path won every pair.

    python bench/infer_bench.py [--pairs 5] [--repeats 5] [--warmup 2] [--batches 1440 691 180 1] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _timed(fn, repeats: int) -> float:
    """ms per call of ``repeats`` back-to-back calls (one call of ~1 ms is at
    the mercy of a single scheduling hiccup), ending in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeats


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5,
                    help="evaluations (batch 1: calls) per timing, run back to back; times are per evaluation")
    ap.add_argument("--sequences", type=int, default=6912)
    ap.add_argument("--batches", type=int, nargs="+", default=[1440, 691, 180, 1],
                    help="batch sizes; 1 times single calls on one sequence, any other size whole evaluations")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)

    from pytorch_distributed_rnn_amd.data.motion import synthetic_motion
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    from pytorch_distributed_rnn_amd.train import fused_eval
    from pytorch_distributed_rnn_amd.train.formatter import TrainingMessageFormatter
    from pytorch_distributed_rnn_amd.train.trainer import Trainer

    logging.getLogger().setLevel(logging.WARNING)  # the evaluation lines are not what is timed
    dev = torch.device("cuda", 0)
    train, _, _ = synthetic_motion(n_train=args.sequences, n_validation=2, n_test=2, seed=0)
    fmt = TrainingMessageFormatter(1)
    lines = []
    for cell in ("lstm", "gru"):
        torch.manual_seed(0)
        model = MotionModel(9, 32, 2, 6, cell=cell)
        trainer = Trainer(model, train, batch_size=1440, learning_rate=2.5e-3, device=dev, warmup=False)
        assert fused_eval.supported(trainer.model, dev), "the fused inference path does not serve the flagship model"
        one = train.features[:1].to(dev).contiguous()

        def evaluate(loader, fused):
            os.environ["PDRNN_FUSED_EVAL"] = "1" if fused else "0"
            return trainer._evaluate(loader, fmt, epoch=0)

        def single(fused):
            if fused:
                out = trainer.model.predict(one)
            else:
                with torch.no_grad():
                    out = trainer.model(one)
            torch.cuda.synchronize()
            return out

        trainer.model.eval()
        for bs in args.batches:
            if bs == 1:
                run = {True: lambda: single(True), False: lambda: single(False)}
                what = "one predict call on one sequence"
            else:
                loader = trainer._get_data_loader(train, batch_size=bs)
                run = {True: lambda l=loader: evaluate(l, True), False: lambda l=loader: evaluate(l, False)}
                what = f"evaluation of {args.sequences} sequences in {len(loader)} batches"
            for _ in range(args.warmup):
                run[False](), run[True]()
            torch.cuda.synchronize()
            pairs = [(_timed(run[False], args.repeats), _timed(run[True], args.repeats)) for _ in range(args.pairs)]
            old, new = [p[0] for p in pairs], [p[1] for p in pairs]
            rec = {"cell": cell, "batch": bs, "what": what,
                   "pairs_ms": [[round(a, 4), round(b, 4)] for a, b in pairs],
                   "forward_ms": {"median": round(statistics.median(old), 4), "min": round(min(old), 4),
                                  "max": round(max(old), 4)},
                   "fused_ms": {"median": round(statistics.median(new), 4), "min": round(min(new), 4),
                                "max": round(max(new), 4)},
                   "speedup_of_medians": round(statistics.median(old) / statistics.median(new), 3),
                   "fused_wins_every_pair": all(b < a for a, b in pairs)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.environ.pop("PDRNN_FUSED_EVAL", None)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
