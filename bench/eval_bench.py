#!/usr/bin/env python
"""Char-LM held-out evaluation at the ``charlm`` configuration (2 x 1024 LSTM,
embed 256, vocabulary 256, bf16; 128 streams x 512-token windows).

Two measurements, one JSON line each:

``head``  the fused vocabulary head + log-softmax + NLL kernel
          (kernels/head_nll.hip) against the unfused pair it replaces, the
          in-tree ``linear`` (16-bit logits written to memory) followed by
          ``xent_fwd`` without gradient, on the same random operands at
          N = 128 x 512 rows.  Both run in one process and alternate after a
          warm-up; a timing is ``--iters`` back-to-back calls between two
          device events.  Reports the pairs, medians, minima and the ratio
          fused / unfused of the medians, and how far the two mean losses are
          apart (the unfused one rounds its logits to 16 bits).
``evaluate``  tokens/s of ``LMTrainer.evaluate`` over ``--windows`` windows:
          whole calls, each ending in its one host read.

    python bench/eval_bench.py [--rounds 7] [--iters 20] [--windows 8] [--repeats 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--skip", choices=("head", "evaluate"), default=None)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)

    from pytorch_distributed_rnn_amd import _ext
    from pytorch_distributed_rnn_amd.data.charlm import CharCorpus
    from pytorch_distributed_rnn_amd.models.charlm import CharLM
    from pytorch_distributed_rnn_amd.ops import head_nll as hn
    from pytorch_distributed_rnn_amd.ops import shadow as sh
    from pytorch_distributed_rnn_amd.ops.gemm import linear
    from pytorch_distributed_rnn_amd.train.lm import LMTrainer

    assert torch.cuda.is_available(), "eval_bench needs the GPU"
    dev = torch.device("cuda", 0)
    mod = _ext.native(dev)
    cdt = torch.bfloat16
    B, T, H, V = args.batch, args.seq_len, args.hidden, args.vocab
    lines = []

    if args.skip != "head":
        N = B * T
        g = torch.Generator(device=dev).manual_seed(0)
        h = torch.randn(N, H, device=dev, generator=g).to(cdt)
        w = torch.randn(V, H, device=dev, generator=g) / H ** 0.5
        b = torch.randn(V, device=dev, generator=g)
        labels = torch.randint(0, V, (N,), device=dev, generator=g)
        w16 = sh.cast(w, cdt)
        assert hn.supported(H, V, cdt, dev)
        accum = hn.new_accum(dev)

        def fused():
            return mod.head_nll(h, w16, b, labels, -100, accum)

        def unfused():
            with torch.no_grad():
                logits = linear(h, w, b)  # [N, V] in bf16: written, then read by the loss
                return mod.xent_fwd(logits, labels, -100, False)[0]

        def timed(fn) -> float:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) * 1e3 / args.iters  # us per call

        for _ in range(args.warmup):
            stats, _ = unfused(), fused()
        accum.zero_()
        fused()
        torch.cuda.synchronize()
        fused_loss = float(accum[0] / accum[1])
        pairs = [(timed(unfused), timed(fused)) for _ in range(args.rounds)]
        old, new = [p[0] for p in pairs], [p[1] for p in pairs]
        # what the fused kernel must move and compute: h once, W once per workgroup (L2), 2 N V H flop
        flop, hbytes = 2.0 * N * V * H, 2.0 * N * H
        rec = {"bench": "head", "N": N, "H": H, "V": V, "dtype": "bf16", "iters": args.iters,
               "pairs_us": [[round(a, 1), round(c, 1)] for a, c in pairs],
               "unfused_us": {"median": round(statistics.median(old), 1), "min": round(min(old), 1), "max": round(max(old), 1)},
               "fused_us": {"median": round(statistics.median(new), 1), "min": round(min(new), 1), "max": round(max(new), 1)},
               "fused_over_unfused_medians": round(statistics.median(new) / statistics.median(old), 4),
               "fused_wins_every_pair": all(c < a for a, c in pairs),
               "fused_tflops": round(flop / statistics.median(new) / 1e6, 1),
               "fused_h_gbytes_per_s": round(hbytes / statistics.median(new) / 1e3, 1),
               "mean_loss_fused": round(fused_loss, 6), "mean_loss_unfused": round(float(stats[0]), 6)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del h, labels

    if args.skip != "evaluate":
        torch.manual_seed(0)
        corpus = CharCorpus.synthetic(B * (T * args.windows + 1), V, seed=0)
        tr = LMTrainer(CharLM(V, 256, H, args.layers, 0.0, cdt), corpus, B, T, device=dev, log_interval=0)
        tr.evaluate(corpus, B, T)  # warm-up: every shape of the timed calls
        runs = [tr.evaluate(corpus, B, T) for _ in range(args.repeats)]
        rate = [r["tokens_per_sec"] for r in runs]
        rec = {"bench": "evaluate", "model": f"{args.layers}x{H} E256 V{V} bf16", "batch": B, "seq_len": T,
               "windows": args.windows, "tokens": runs[0]["tokens"], "loss": round(runs[0]["loss"], 6),
               "tokens_per_sec": {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1),
                                  "max": round(max(rate), 1)},
               "ms_per_window": round(statistics.median(r["duration"] for r in runs) * 1e3 / args.windows, 3),
               **_ext.persist_stats()}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
