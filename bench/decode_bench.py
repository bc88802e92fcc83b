#!/usr/bin/env python
"""Char-LM generation: the fused decode kernels against the reference path.

Times ``CharLM.generate`` at the char-LM configuration (2 x 1024 LSTM, embed
256, vocabulary 256, bf16; 512 tokens after a one-token prompt) at B = 1, 4
and 16 streams.  Both paths run in one process and alternate after a warm-up:
the fused path (kernels/lstm_decode.hip: layers + 1 launches per token, no
host read) and the reference path (``PDRNN_KERNELS=torch`` is NOT what is
meant: ``generate``'s token-by-token loop over ``forward`` on the training
kernels, reached by making ``ops.decode.supported`` answer no).  Every timing
is one whole ``generate`` call ending in a device synchronise and a host copy
of the tokens.  Prints one JSON line per B: the pairs in microseconds per
token, both medians and ranges, and whether the fused path won every pair.

``--profile-one B``: instead, one warmed-up fused ``generate`` call and one
reference call of ``--tokens`` tokens (for a ``rocprofv3 --kernel-trace
--stats`` run of its own; the per-token kernel table is its totals over the
token count).

``--top-k K`` / ``--top-p P`` / ``--logprobs``: both paths sample through the
filters (and return the tokens' log-probabilities); the defaults are off, which
is the plain sampler the figures of profiles/r11 were taken with.

``--beam-width W ...``: beam search instead (``CharLM.beam_search``, one
prompt): per width, the reference path, the fused path and plain fused
sampling of W streams alternate in one process after the warm-up; one JSON
line per width.

    python bench/decode_bench.py [--pairs 5] [--warmup 2] [--tokens 512] [--batches 1 4 16] [--out FILE]
                                 [--top-k 40] [--top-p 0.9] [--logprobs] [--beam-width 1 4 16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def beam(args, model, dec, dev, cdt, generate) -> int:
    """``--beam-width``: per width W one JSON line.  After a warm-up, three
    calls alternate ``--pairs`` times in one process: ``CharLM.beam_search`` on
    the reference path (``beam_reference`` over ``forward``, reached by making
    ``ops.decode.beam_supported`` answer no), on the fused kernels, and plain
    fused sampling of W streams.  Microseconds per position of one prompt's
    search."""
    import warnings
    real = dec.beam_supported
    prompt = torch.zeros(1, 1, dtype=torch.int64, device=dev)

    def search(W, fused: bool):
        dec.beam_supported = real if fused else (lambda *a, **k: False)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                return model.beam_search(prompt, args.tokens, W)[0].cpu()
        finally:
            dec.beam_supported = real

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.tokens

    def summary(xs):
        return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}

    lines = []
    for W in args.beam_width:
        assert real(1, W, args.hidden, args.embed, args.vocab, args.layers, cdt, dev), f"the decode kernels do not cover W = {W}"
        streams = torch.zeros(W, 1, dtype=torch.int64, device=dev)
        calls = {"reference": lambda: search(W, False), "fused": lambda: search(W, True),
                 "sampling": lambda: generate(streams, True)}
        for _ in range(args.warmup):
            outs = {k: f() for k, f in calls.items()}
        rounds = [{k: timed(f) for k, f in calls.items()} for _ in range(args.pairs)]
        rec = {"beam_width": W, "tokens": args.tokens,
               "model": f"{args.layers}x{args.hidden} E{args.embed} V{args.vocab} {args.dtype}",
               "rounds_us_per_token": [{k: round(v, 2) for k, v in r.items()} for r in rounds]}
        for k in calls:
            rec[k + "_us_per_token"] = summary([r[k] for r in rounds])
        rec["speedup_of_medians"] = round(rec["reference_us_per_token"]["median"] / rec["fused_us_per_token"]["median"], 2)
        rec["fused_wins_every_round"] = all(r["fused"] < r["reference"] for r in rounds)
        # (not a pass criterion: how long the two paths' best hypotheses agree)
        rec["best_equal_prefix"] = int((outs["fused"][0, 0] == outs["reference"][0, 0]).long().cumprod(0).sum())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--embed", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0, help="0: off")
    ap.add_argument("--top-p", type=float, default=1.0, help="1: off")
    ap.add_argument("--logprobs", action="store_true", help="also return the tokens' log-probabilities")
    ap.add_argument("--beam-width", type=int, nargs="+", default=None, metavar="W",
                    help="time beam search at these widths instead (one prompt per call)")
    ap.add_argument("--profile-one", type=int, default=None, metavar="B")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)

    from pytorch_distributed_rnn_amd.models.charlm import CharLM
    from pytorch_distributed_rnn_amd.ops import decode as dec

    assert torch.cuda.is_available(), "decode_bench needs the GPU"
    dev = torch.device("cuda", 0)
    cdt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    torch.manual_seed(0)
    model = CharLM(args.vocab, args.embed, args.hidden, args.layers, compute_dtype=cdt).to(dev).eval()
    real_supported = dec.supported

    def generate(prompt, fused: bool):
        # the reference path is generate's own: the shape reported as not covered
        dec.supported = real_supported if fused else (lambda *a, **k: False)
        try:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                out = model.generate(prompt, args.tokens, temperature=args.temperature, seed=1, top_k=args.top_k,
                                     top_p=args.top_p, return_logprobs=args.logprobs)
            tokens = out[0] if args.logprobs else out
            return tokens.cpu()  # (the host read a caller ends with)
        finally:
            dec.supported = real_supported

    def timed(prompt, fused: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate(prompt, fused)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.tokens

    if args.beam_width:
        return beam(args, model, dec, dev, cdt, generate)

    if args.profile_one is not None:
        prompt = torch.zeros(args.profile_one, 1, dtype=torch.int64, device=dev)
        assert real_supported(args.profile_one, args.hidden, args.embed, args.vocab, args.layers, cdt, dev)
        for _ in range(args.warmup):
            generate(prompt, False), generate(prompt, True)
        print(json.dumps({"profile_one": args.profile_one, "tokens": args.tokens, "top_k": args.top_k,
                          "top_p": args.top_p, "logprobs": args.logprobs,
                          "reference_us_per_token": round(timed(prompt, False), 2),
                          "fused_us_per_token": round(timed(prompt, True), 2)}), flush=True)
        return 0

    lines = []
    for B in args.batches:
        prompt = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        assert real_supported(B, args.hidden, args.embed, args.vocab, args.layers, cdt, dev), \
            f"the decode kernels do not cover B = {B}"
        for _ in range(args.warmup):
            ref, new = generate(prompt, False), generate(prompt, True)
        pairs = [(timed(prompt, False), timed(prompt, True)) for _ in range(args.pairs)]
        old, fused = [p[0] for p in pairs], [p[1] for p in pairs]
        rec = {"B": B, "tokens": args.tokens, "model": f"{args.layers}x{args.hidden} E{args.embed} V{args.vocab} {args.dtype}",
               "top_k": args.top_k, "top_p": args.top_p, "logprobs": args.logprobs,
               "pairs_us_per_token": [[round(a, 2), round(b, 2)] for a, b in pairs],
               "reference_us_per_token": {"median": round(statistics.median(old), 2), "min": round(min(old), 2),
                                          "max": round(max(old), 2)},
               "fused_us_per_token": {"median": round(statistics.median(fused), 2), "min": round(min(fused), 2),
                                      "max": round(max(fused), 2)},
               "speedup_of_medians": round(statistics.median(old) / statistics.median(fused), 2),
               "fused_wins_every_pair": all(b < a for a, b in pairs),
               # both paths sample by one rule: how long their token streams agree says how far the
               # two paths' logits stay within the rule's resolution of each other (not a pass criterion)
               "tokens_equal_prefix": int((ref == new).all(0).long().cumprod(0).sum())}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
