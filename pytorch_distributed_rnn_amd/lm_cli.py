"""Char-LM training, evaluation and generation entry point (BASELINE config 4).

    python -m pytorch_distributed_rnn_amd.lm_cli --hidden 1024 --layers 2 --seq-len 512 \\
        --batch-size 64 --max-steps 100 local
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m pytorch_distributed_rnn_amd.lm_cli ... distributed

    python -m pytorch_distributed_rnn_amd.lm_cli --checkpoint out/charlm-epoch0.pt \\
        --prompt "The " --num-tokens 256 --temperature 0.8 --top-k 40 --top-p 0.9 --stop-token 10 \\
        --samples 4 generate
    python -m pytorch_distributed_rnn_amd.lm_cli --checkpoint out/charlm-epoch0.pt \\
        --prompt "The " --num-tokens 64 --beam-width 8 --samples 3 --stop-token 10 --length-penalty 0.7 generate

    python -m pytorch_distributed_rnn_amd.lm_cli --text corpus.txt --validation-fraction 0.1 \\
        --checkpoint-directory out local
    python -m pytorch_distributed_rnn_amd.lm_cli --checkpoint out/charlm-best.pt --text test.txt evaluate

Data: ``--text FILE`` (bytes) or a synthetic corpus (default).  ``--batch-size``
is global (strong scaling) unless ``--weak-scaling``.  ``--validation-fraction
F`` holds the last F of the token stream out of training: every epoch then
ends with its loss, bits per character and accuracy (``val_*`` in the
history), and ``charlm-best.pt`` keeps the checkpoint with the lowest
``val_loss``.  ``generate`` and ``evaluate`` rebuild the model from the
checkpoint alone (only ``--dtype`` is read from the command line); ``generate``
samples ``--samples`` continuations of the prompt -- or, with ``--beam-width
W``, searches for the most likely ones with W beams and prints the ``--samples``
best (``CharLM.beam_search``; no sampling flags then) --, ``evaluate`` scores
``--text`` or the synthetic corpus (with ``--validation-fraction`` its held-out
tail only: a training run's validation figure again, from its checkpoint).
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from typing import Optional

import torch

from .data.charlm import CharCorpus
from .models.charlm import CharLM
from .train.lm import LMTrainer

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="char-LM LSTM training and generation")
    p.add_argument("--text", default=None)
    p.add_argument("--synthetic-tokens", type=int, default=4_000_000)
    p.add_argument("--vocab", type=int, default=256)
    p.add_argument("--embed", type=int, default=256)
    p.add_argument("--hidden", type=int, default=1024)
    p.add_argument("--layers", type=int, default=2)
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--seq-len", type=int, default=512)
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--weak-scaling", action="store_true")
    p.add_argument("--learning-rate", type=float, default=2e-3)
    p.add_argument("--grad-clip", type=float, default=1.0)
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--dtype", choices=sorted(DTYPES), default="bf16")
    p.add_argument("--backend", default=None)
    p.add_argument("--bucket-mb", type=float, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log", default="INFO")
    p.add_argument("--log-interval", type=int, default=50)
    p.add_argument("--device", default=None)
    p.add_argument("--history-file", default=None)
    p.add_argument("--checkpoint-directory", default=None, help="save <dir>/charlm-epoch<k>.pt after every epoch")
    p.add_argument("--resume", default=None, help="checkpoint to continue from")
    p.add_argument("--trace", action="store_true", help="roctx / torch.profiler ranges around step phases")
    p.add_argument("--profile", default=None, help="torch.profiler capture of the run into this directory")
    p.add_argument("--validation-fraction", type=float, default=0.0,
                   help="hold the last F of the token stream out of training and evaluate it after every epoch")
    p.add_argument("--eval-batch-size", type=int, default=16, help="parallel streams of an evaluation")
    g = p.add_argument_group("generate / evaluate")
    g.add_argument("--checkpoint", default=None, help="the trained model to sample from or to score with (required)")
    g.add_argument("--prompt", default=None, help="text the samples continue (UTF-8 bytes are the tokens)")
    g.add_argument("--prompt-file", default=None, help="the prompt's bytes from a file instead")
    g.add_argument("--num-tokens", type=int, default=256)
    g.add_argument("--temperature", type=float, default=1.0, help="0: greedy")
    g.add_argument("--top-k", type=int, default=0, help="generate: sample among the k most likely bytes (ties with "
                                                       "the k-th kept); 0: off")
    g.add_argument("--top-p", type=float, default=1.0, help="generate: then among the most likely of them that hold "
                                                         "this share of their probability; 1: off")
    g.add_argument("--stop-token", type=int, default=None, help="generate: a byte value; a sample ends before its first one")
    g.add_argument("--logprobs-file", default=None, help="generate: write every sample's token log-probabilities "
                                                         "(under the filtered distribution) and their sum here as JSON")
    g.add_argument("--samples", type=int, default=1, help="generate: samples drawn; with --beam-width the hypotheses "
                                                          "printed, best first (at most the width)")
    g.add_argument("--beam-width", type=int, default=0, help="generate: beam search with this many beams (1..16) "
                                                              "instead of sampling; 0: off")
    g.add_argument("--length-penalty", type=float, default=0.0, help="generate, beam search: rank the final hypotheses "
                                                                       "by score / length^A; 0: off")
    g.add_argument("--output", default=None, help="generate: write the samples' raw bytes here, one after another; "
                                                   "evaluate: write the figures here as JSON")
    p.add_argument("mode", choices=("local", "distributed", "generate", "evaluate"))
    return p


def load_corpus(args) -> CharCorpus:
    return (CharCorpus.from_text(args.text) if args.text
            else CharCorpus.synthetic(args.synthetic_tokens, args.vocab, seed=args.seed))


def split_corpus(corpus: CharCorpus, fraction: float):
    """(training part, held-out part or None): the last ``fraction`` of the
    token stream is held out; at 0 the training part is the corpus itself."""
    if fraction == 0:
        return corpus, None
    n_val = int(len(corpus) * fraction)
    cut = len(corpus) - n_val
    return CharCorpus(corpus.tokens[:cut], corpus.vocab_size), CharCorpus(corpus.tokens[cut:], corpus.vocab_size)


def generate(args):
    """``generate``: rebuild the model a checkpoint describes and sample
    ``--samples`` continuations of the prompt, ``--num-tokens`` tokens each.
    The samples are the rows of one batch, so they differ by their row index
    in the sampling hash; the same ``--seed`` gives the same text again.
    ``--beam-width W``: one beam search instead, its ``--samples`` best
    hypotheses, best first; ``sum`` in ``--logprobs-file`` is a hypothesis's
    score."""
    from .models.charlm import charlm_from_state_dict
    from .train import checkpoint as ckpt
    from .train.trainer import default_device
    if not args.checkpoint:
        raise SystemExit("generate: --checkpoint is required")
    if args.prompt is not None and args.prompt_file is not None:
        raise SystemExit("generate: give --prompt or --prompt-file, not both")
    if args.samples < 1 or args.num_tokens < 0 or args.temperature < 0:
        raise SystemExit("generate: --samples >= 1, --num-tokens >= 0 and --temperature >= 0")
    if args.top_k < 0 or not 0 < args.top_p <= 1:
        raise SystemExit("generate: --top-k >= 0 and --top-p in (0, 1]")
    beam = args.beam_width != 0
    if beam and not (1 <= args.beam_width <= 16 and args.samples <= args.beam_width and args.num_tokens >= 1):
        raise SystemExit("generate: --beam-width in [1, 16], --samples <= --beam-width and --num-tokens >= 1")
    if beam and (args.top_k != 0 or args.top_p != 1.0 or args.temperature != 1.0):
        raise SystemExit("generate: --beam-width searches, it does not sample: no --top-k, --top-p or --temperature")
    if not beam and args.length_penalty != 0:
        raise SystemExit("generate: --length-penalty needs --beam-width")
    if args.prompt_file is not None:
        with open(args.prompt_file, "rb") as f:
            prompt = f.read()
    else:
        prompt = (args.prompt if args.prompt is not None else "\n").encode("utf-8")
    if not prompt:
        raise SystemExit("generate: the prompt is empty")
    model = charlm_from_state_dict(ckpt.read_checkpoint(args.checkpoint)["model_state"], DTYPES[args.dtype])
    if model.vocab_size > 256:
        raise SystemExit(f"generate: a vocabulary of {model.vocab_size} entries is not bytes")
    if max(prompt) >= model.vocab_size:
        raise SystemExit(f"generate: the prompt holds byte {max(prompt)}, the model's vocabulary is {model.vocab_size}")
    if args.stop_token is not None and not 0 <= args.stop_token < model.vocab_size:
        raise SystemExit(f"generate: --stop-token {args.stop_token} is outside the model's vocabulary of {model.vocab_size}")
    device = torch.device(args.device) if args.device else default_device()
    model = model.to(device).eval()
    want_lp = args.logprobs_file is not None
    sums = None
    if beam:
        # the --samples best hypotheses of one search; a beam that found no continuation (score -inf) is left out
        out = model.beam_search(torch.tensor([list(prompt)], dtype=torch.int64), args.num_tokens, args.beam_width,
                                stop=args.stop_token, length_penalty=args.length_penalty, return_logprobs=want_lp)
        keep = [i for i, s in enumerate(out[1][0].cpu().tolist()[:args.samples]) if s != float("-inf")]
        tokens, lengths = [out[0][0].cpu().tolist()[i] for i in keep], [out[2][0].cpu().tolist()[i] for i in keep]
        sums = [out[1][0].double().cpu().tolist()[i] for i in keep]
        logprobs = out[3][0].double().cpu()[keep] if want_lp else None
    else:
        out = model.generate(torch.tensor(list(prompt), dtype=torch.int64).repeat(args.samples, 1), args.num_tokens,
                             temperature=args.temperature, seed=args.seed, top_k=args.top_k, top_p=args.top_p,
                             stop=args.stop_token, return_logprobs=want_lp, return_lengths=True)
        tokens, lengths = out[0].cpu().tolist(), out[-1].cpu().tolist()
        logprobs = out[1].double().cpu() if want_lp else None
    # a sample ends before its stop byte; its log-probs include the stop's
    samples = [bytes(row[:n - 1] if n and row[n - 1] == args.stop_token else row[:n]) for row, n in zip(tokens, lengths)]
    if want_lp:
        if sums is None:
            sums = [float(lp[:n].sum()) for lp, n in zip(logprobs, lengths)]
        with open(args.logprobs_file, "w") as f:
            json.dump({"samples": [{"length": n, "logprobs": lp[:n].tolist(), "sum": s}
                                   for lp, n, s in zip(logprobs, lengths, sums)]}, f)
    if args.output:
        with open(args.output, "wb") as f:
            f.write(b"".join(samples))
    for s in samples:
        print(s.decode("utf-8", errors="replace"))
    return samples


def _check_split(args, mode: str, corpus: CharCorpus, held: Optional[CharCorpus]) -> None:
    if not 0 <= args.validation_fraction < 1:
        raise SystemExit(f"{mode}: --validation-fraction must be in [0, 1)")
    if args.eval_batch_size < 1:
        raise SystemExit(f"{mode}: --eval-batch-size >= 1")
    if held is not None and len(held) < 2 * args.eval_batch_size:
        raise SystemExit(f"{mode}: the held-out part has {len(held)} tokens, too few for {args.eval_batch_size} streams")
    if len(corpus) < 2:
        raise SystemExit(f"{mode}: the corpus has {len(corpus)} tokens")


def evaluate(args):
    """``evaluate``: rebuild the model a checkpoint describes and score a text
    with it: loss (nats per token), bits per character and next-token accuracy
    over ``--eval-batch-size`` parallel streams of ``--seq-len`` windows, the
    state carried from window to window."""
    from .models.charlm import charlm_from_state_dict
    from .train import checkpoint as ckpt
    from .train.trainer import default_device
    if not args.checkpoint:
        raise SystemExit("evaluate: --checkpoint is required")
    if args.seq_len < 1:
        raise SystemExit("evaluate: --seq-len >= 1")
    if not 0 <= args.validation_fraction < 1:
        raise SystemExit("evaluate: --validation-fraction must be in [0, 1)")
    corpus, held = split_corpus(load_corpus(args), args.validation_fraction)
    _check_split(args, "evaluate", corpus, held)
    scored = held if held is not None else corpus
    if len(scored) < 2 * args.eval_batch_size:
        raise SystemExit(f"evaluate: {len(scored)} tokens are too few for {args.eval_batch_size} streams")
    model = charlm_from_state_dict(ckpt.read_checkpoint(args.checkpoint)["model_state"], DTYPES[args.dtype])
    if int(scored.tokens.max()) >= model.vocab_size:
        raise SystemExit(f"evaluate: the text holds token {int(scored.tokens.max())}, the model's vocabulary is "
                         f"{model.vocab_size}")
    device = torch.device(args.device) if args.device else default_device()
    trainer = LMTrainer(model, scored, args.eval_batch_size, args.seq_len, device=device)
    out = trainer.evaluate(scored, args.eval_batch_size, args.seq_len)
    print(f"loss {out['loss']:.6f} bpc {out['bpc']:.4f} accuracy {out['accuracy']:.4f} tokens {out['tokens']}")
    if args.output:
        with open(args.output, "w") as f:
            json.dump(out, f)
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=args.log, format="%(message)s")
    if args.mode == "generate":
        return generate(args)
    if args.mode == "evaluate":
        return evaluate(args)
    torch.manual_seed(args.seed)
    corpus, held = split_corpus(load_corpus(args), args.validation_fraction)
    _check_split(args, args.mode, corpus, held)
    model = CharLM(corpus.vocab_size, args.embed, args.hidden, args.layers, args.dropout, DTYPES[args.dtype])
    device = torch.device(args.device) if args.device else None
    trainer = LMTrainer(model, corpus, args.batch_size, args.seq_len, args.learning_rate, device=device,
                        distributed=args.mode == "distributed", backend=args.backend,
                        grad_clip=args.grad_clip, log_interval=args.log_interval,
                        bucket_cap_mb=args.bucket_mb, weak_scaling=args.weak_scaling,
                        validation=held, eval_batch=args.eval_batch_size)
    start = trainer.resume(args.resume) if args.resume else 0
    history = []
    best = float("inf")
    from .utils import tracing
    if args.trace:
        tracing.enable(True)
    with tracing.profile(args.profile, trainer.rank):
        for e in range(start, start + args.epochs):
            h = trainer.train_epoch(e, args.max_steps)
            history.append(h)
            if args.checkpoint_directory:
                from pathlib import Path
                trainer.save(Path(args.checkpoint_directory) / f"charlm-epoch{e}.pt", e, h["loss"])
                if "val_loss" in h and h["val_loss"] < best:  # (rank 0 alone evaluates)
                    best = h["val_loss"]
                    trainer.save(Path(args.checkpoint_directory) / "charlm-best.pt", e, h["loss"])
    if trainer.rank == 0 and args.history_file:
        with open(args.history_file, "w") as f:
            json.dump(history, f)
    if args.mode == "distributed":
        from .parallel import env
        env.shutdown()
    return history


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
