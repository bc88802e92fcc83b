"""Character-level LSTM language model (BASELINE config 4: 2-layer LSTM,
hidden 1024, seq_len 512, DDP) and the stacked bidirectional LSTM encoder
(BASELINE config 5: hidden 4096, fp16).

Neither model exists in the reference (no GRU / embedding /
char-LM there); they reuse its building blocks -- ``nn.LSTM``-compatible
layers whose forward runs on the framework's kernels -- and make
``_reset_hidden_state`` real (the reference's is dead code,
reference: src/motion/trainer/base.py:161-162) for truncated BPTT.

Precision: parameters are fp32 masters; the recurrent stack, the embedding
output and the vocabulary projection run in ``compute_dtype`` (bf16 / fp16 on
MI355X), the loss in fp32.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Tuple

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from ..ops.embedding import embedding
from ..ops.gemm import linear
from .rnn import LSTM


class CharLM(nn.Module):
    def __init__(self, vocab_size: int = 256, embed_dim: int = 256, hidden_dim: int = 1024,
                 num_layers: int = 2, dropout: float = 0.0, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self.vocab_size = vocab_size
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        self.compute_dtype = compute_dtype
        self.embedding = nn.Embedding(vocab_size, embed_dim)
        self.lstm = LSTM(embed_dim, hidden_dim, num_layers, batch_first=False, dropout=dropout)
        self.fc = nn.Linear(hidden_dim, vocab_size)
        self._state: Optional[Tuple[Tensor, Tensor]] = None

    def reset_hidden_state(self) -> None:
        """Start a new TBPTT stream (called at every epoch start)."""
        self._state = None

    def _cdt(self, device) -> torch.dtype:
        return self.compute_dtype if device.type == "cuda" else torch.float32

    def forward(self, tokens: Tensor, state: Optional[Tuple[Tensor, Tensor]] = None,
                carry: bool = False) -> Tensor:
        """tokens [B, T] -> logits [T, B, V] (sequence-first, compute dtype).

        ``carry=True`` continues from (and updates) the detached state of the
        previous segment -- truncated BPTT over a long stream."""
        cdt = self._cdt(tokens.device)
        x = embedding(tokens.t(), self.embedding.weight, out_dtype=cdt)      # [T, B, E]
        if state is None and carry:
            state = self._state
        out, (hn, cn) = self.lstm(x, state)
        if carry:
            self._state = (hn.detach(), cn.detach())
        return linear(out, self.fc.weight, self.fc.bias)  # in-tree GEMM head (ops/gemm.py)

    def _step(self, tokens: Tensor, state):
        """One ``forward`` call from an explicit state -> (last position's
        logits [B, V], new state), through the carry the training loop uses."""
        self._state = state
        logits = self.forward(tokens, carry=True)
        return logits[-1], self._state

    @contextlib.contextmanager
    def _decoding(self, what: str, prompt: Tensor, state, forced: Optional[Tensor] = None):
        """What ``generate`` and ``beam_search`` do around their positions:
        ``prompt`` [B, P] goes to the device (ValueError unless P >= 1, or where
        it or ``forced``, on the CPU, hold tokens outside the vocabulary), the
        model runs in eval mode and ``prompt[:, :-1]`` through ``_step`` from
        ``state``; the training mode and the truncated-BPTT carry are put back
        on the way out.  Yields (P, the first input tokens [B], the state after
        the prefix, the compute dtype, whether the LSTM is one the decode
        kernels know: biases, one direction, no projection)."""
        if prompt.dim() != 2 or prompt.shape[1] < 1:
            raise ValueError(f"{what}: prompt must be [B, P] with P >= 1")
        dev = self.embedding.weight.device
        prompt = prompt.to(dev, torch.int64)
        for name, t in (("prompt", prompt), ("forced", forced)):
            if t is not None and t.device.type == "cpu" and t.numel() and not (0 <= int(t.min()) and int(t.max()) < self.vocab_size):
                raise ValueError(f"{what}: {name} holds tokens outside the vocabulary")
        P = prompt.shape[1]
        kept, training = self._state, self.training
        self.eval()
        try:
            if P > 1:
                _, state = self._step(prompt[:, :-1], state)
            plain = self.lstm.bias and not self.lstm.bidirectional and self.lstm.proj_size == 0
            yield P, prompt[:, -1], state, self._cdt(dev), plain
        finally:
            self._state = kept
            self.train(training)

    @torch.no_grad()
    def generate(self, prompt: Tensor, num_tokens: int, temperature: float = 1.0, seed: int = 0,
                 state: Optional[Tuple[Tensor, Tensor]] = None, forced: Optional[Tensor] = None,
                 return_logits: bool = False, return_state: bool = False, top_k: int = 0, top_p: float = 1.0,
                 stop: Optional[int] = None, return_logprobs: bool = False, return_lengths: bool = False):
        """Sample ``num_tokens`` tokens after ``prompt`` [B, P] (P >= 1) ->
        tokens [B, num_tokens] int64 (, logits [B, num_tokens, V] fp32)
        (, log-probs [B, num_tokens] fp32) (, lengths [B] int64)
        (, (h, c) [layers, B, H], c in fp32 on the fused path).

        The rule is ops/decode.py's: ``token = argmax(logits / temperature +
        Gumbel noise)``, the noise a hash of (seed, row of the batch, position
        counted from the prompt's start, vocabulary entry); temperature 0 is
        greedy.  ``prompt[:, :-1]`` runs through ``forward`` from ``state``
        (zeros when None); the last prompt token is the first input.
        ``forced`` [B, num_tokens] replaces every position's input token (the
        sampled ones are still returned): scoring a given continuation.

        ``top_k`` / ``top_p`` restrict the draw to the k largest logits (ties
        with the k-th kept) and then to the smallest head of them that holds
        ``top_p`` of their probability; the log-probs are the drawn tokens'
        under that kept, renormalised distribution (ops/decode.py: the rule).
        ``stop``: from a row's first sampled ``stop`` token on, its tokens are
        ``stop`` and its log-probs 0; ``lengths`` counts a row's tokens up to
        and including that first ``stop`` (``num_tokens`` without one).  The
        rows are independent and all launches are enqueued up front, so
        ``stop`` is applied to the finished batch, on the device, with no host
        read; the logits and the state are those of the full run.

        On the GPU, 16-bit models the decode kernels cover run on them
        (kernels/lstm_decode.hip; more than 16 rows as independent groups of
        16); everything else takes the reference path, ``forward`` one token at
        a time -- an error under ``PDRNN_KERNELS=hip-strict``.  Dropout is off
        and the truncated-BPTT carry is left as it was."""
        from .. import _ext
        from ..ops import decode as dec
        dev = self.embedding.weight.device
        forced = forced.to(dev, torch.int64) if forced is not None else None
        N = int(num_tokens)
        if forced is not None and prompt.dim() == 2 and tuple(forced.shape) != (prompt.shape[0], N):
            raise ValueError("generate: forced must be [B, num_tokens]")
        dec.check_filters(top_k, top_p)
        if stop is not None and forced is not None:
            raise ValueError("generate: stop and forced exclude each other")
        if stop is not None and not 0 <= int(stop) < self.vocab_size:
            raise ValueError(f"generate: stop token {stop} is outside the vocabulary")
        V, E, H, L = self.vocab_size, self.embedding.embedding_dim, self.hidden_dim, self.num_layers
        with self._decoding("generate", prompt, state, forced) as (P, first, state, cdt, plain):
            B = first.shape[0]
            logprobs = None
            filt = dict(top_k=top_k, top_p=top_p, return_logprobs=return_logprobs)
            if N > 0 and plain and dec.supported(min(B, dec.MAX_STREAMS), H, E, V, L, cdt, dev):
                outs = []
                for b0 in range(0, B, dec.MAX_STREAMS):
                    rows = slice(b0, min(b0 + dec.MAX_STREAMS, B))
                    outs.append(dec.decode(
                        self.embedding.weight, self.lstm._weights(), self.fc.weight, self.fc.bias, cdt,
                        state[0][:, rows] if state is not None else None, state[1][:, rows] if state is not None else None,
                        first[rows], N, temperature=temperature, seed=seed, stream0=b0, pos0=P,
                        forced=forced[rows] if forced is not None else None, return_logits=return_logits, **filt))
                if len(outs) == 1:
                    tokens, logits, h, c = outs[0][:4]
                    logprobs = outs[0][4] if return_logprobs else None
                else:
                    tokens = torch.cat([o[0] for o in outs], 0)
                    logits = torch.cat([o[1] for o in outs], 0) if return_logits else None
                    h, c = torch.cat([o[2] for o in outs], 1), torch.cat([o[3] for o in outs], 1)
                    logprobs = torch.cat([o[4] for o in outs], 0) if return_logprobs else None
                state = (h, c)
            else:
                if N > 0:
                    _ext.fallback(f"char-LM decode (B={B}, H={H}, E={E}, V={V}, layers={L}, {cdt})", dev)
                tokens, logits, state, *rest = dec.reference(self._step, state, first, N, temperature=temperature,
                                                             seed=seed, pos0=P, forced=forced,
                                                             return_logits=return_logits, **filt)
                logprobs = rest[0] if return_logprobs else None
                if return_logits and logits is None:  # (no position at all)
                    logits = torch.empty(B, 0, V, device=dev)
        lengths = None
        if stop is not None or return_lengths:
            lengths, past = dec.stop_lengths(tokens, stop)
            if stop is not None:
                tokens = torch.where(past, torch.full_like(tokens, int(stop)), tokens)
                if logprobs is not None:
                    logprobs = torch.where(past, torch.zeros_like(logprobs), logprobs)
        out = ((tokens,) + ((logits,) if return_logits else ()) + ((logprobs,) if return_logprobs else ())
               + ((lengths,) if return_lengths else ()) + ((state,) if return_state else ()))
        return out[0] if len(out) == 1 else out

    @torch.no_grad()
    def beam_search(self, prompt: Tensor, num_tokens: int, beam_width: int, stop: Optional[int] = None,
                    length_penalty: float = 0.0, state: Optional[Tuple[Tensor, Tensor]] = None,
                    return_logprobs: bool = False, return_state: bool = False):
        """The ``beam_width`` most likely continuations of ``prompt`` [B, P]
        (P >= 1) found by beam search -> tokens [B, W, num_tokens] int64 best
        first, scores [B, W] fp32, lengths [B, W] int64 (, per-token log-probs
        [B, W, num_tokens] fp32 along each hypothesis) (, (h, c) [layers,
        B * W, H], row b * W + i hypothesis i's).

        The rule is ops/decode.py's: a hypothesis's score is the sum of its
        tokens' log-probs (softmax of the fp32 logits); ties keep the lower
        source beam, then the lower token; a prompt's unused beams (fewer than
        W continuations exist, or survive) score -inf.  With ``stop`` a
        hypothesis ends at its first ``stop`` token: its score freezes, its
        later tokens are ``stop`` with log-prob 0 and its length counts up to
        and including that ``stop``; the state is the full run's, as in
        ``generate``.  ``length_penalty`` a != 0 re-ranks the final W by score /
        length^a, and that quotient is the score returned.  Deterministic:
        no seed.

        Routing as in ``generate``: ``prompt[:, :-1]`` runs through ``forward``
        from ``state``; 16-bit models the decode kernels cover run on them,
        ``16 // beam_width`` prompts per call; everything else takes the
        reference path, ``forward`` one token at a time -- an error under
        ``PDRNN_KERNELS=hip-strict``.  Dropout is off and the truncated-BPTT
        carry is left as it was."""
        from .. import _ext
        from ..ops import decode as dec
        V, E, H, L = self.vocab_size, self.embedding.embedding_dim, self.hidden_dim, self.num_layers
        dec.check_beam(beam_width, stop, V, num_tokens)
        dev = self.embedding.weight.device
        N, W = int(num_tokens), int(beam_width)
        with self._decoding("beam_search", prompt, state) as (_, first, state, cdt, plain):
            B = first.shape[0]
            per = dec.MAX_STREAMS // W
            if plain and dec.beam_supported(min(B, per), W, H, E, V, L, cdt, dev):
                outs = []
                for b0 in range(0, B, per):
                    rows = slice(b0, min(b0 + per, B))
                    outs.append(dec.beam_decode(
                        self.embedding.weight, self.lstm._weights(), self.fc.weight, self.fc.bias, cdt,
                        state[0][:, rows] if state is not None else None, state[1][:, rows] if state is not None else None,
                        first[rows], N, W, stop=stop, return_logprobs=return_logprobs))
            else:
                _ext.fallback(f"char-LM beam search (B={B}, W={W}, H={H}, E={E}, V={V}, layers={L}, {cdt})", dev)
                o = dec.beam_reference(self._step, state, first, N, W, stop=stop, return_logprobs=return_logprobs)
                outs = [o[:3] + tuple(o[3])]
            hyp, scores = torch.cat([o[0] for o in outs], 0), torch.cat([o[1] for o in outs], 0).float()
            logprobs = torch.cat([o[2] for o in outs], 0).float() if return_logprobs else None
            h, c = torch.cat([o[3] for o in outs], 1), torch.cat([o[4] for o in outs], 1)
        order, lengths, scores = dec.beam_finish(hyp, scores, stop, length_penalty)
        if length_penalty:
            hyp = hyp.gather(1, order[:, :, None].expand_as(hyp))
            if logprobs is not None:
                logprobs = logprobs.gather(1, order[:, :, None].expand_as(logprobs))
            rows = (order + torch.arange(B, device=dev)[:, None] * W).reshape(-1)
            h, c = h.index_select(1, rows), c.index_select(1, rows)
        return ((hyp, scores, lengths) + ((logprobs,) if return_logprobs else ())
                + (((h, c),) if return_state else ()))

    @torch.no_grad()
    def score(self, inputs: Tensor, targets: Tensor, state: Optional[Tuple[Tensor, Tensor]] = None,
              return_state: bool = False, ignore_index: int = -100, accum: Optional[Tensor] = None):
        """Per-token log-probabilities of ``targets`` [B, T] after ``inputs``
        [B, T] -> (logprob [B, T] fp32, pred [B, T] int32) (, (h, c) [layers,
        B, H]); ``logprob`` is 0 where the target is ``ignore_index``, ``pred``
        the argmax of the position's logits (the lowest index on ties).

        The embedding and the LSTM stack run as in ``forward`` from ``state``
        (zeros when None); the vocabulary head, the log-softmax and the NLL are
        one kernel on the top layer's output in place (ops/head_nll.py), with
        the logits in fp32 from the product to the loss -- ``forward`` would
        round them to the compute dtype first.  ``accum`` (fp64 [3], added to:
        sum of -logprob, valid tokens, correct predictions) lets a caller total
        many windows on the device.  Dropout is off; the training mode and the
        truncated-BPTT carry are left as they were."""
        from ..ops.head_nll import head_nll
        if inputs.dim() != 2 or inputs.shape != targets.shape:
            raise ValueError("score: inputs and targets must both be [B, T]")
        dev = self.embedding.weight.device
        inputs, targets = inputs.to(dev, torch.int64), targets.to(dev, torch.int64)
        B, T = inputs.shape
        training = self.training
        self.eval()
        try:
            x = embedding(inputs.t(), self.embedding.weight, out_dtype=self._cdt(dev))  # [T, B, E]
            out, (hn, cn) = self.lstm(x, state)                                          # [T, B, H]
            row_nll, pred, _ = head_nll(out, self.fc.weight, self.fc.bias, targets.t().contiguous(), ignore_index, accum)
        finally:
            self.train(training)
        logprob = -row_nll.view(T, B).t()
        pred = pred.view(T, B).t()
        return (logprob, pred, (hn, cn)) if return_state else (logprob, pred)


def charlm_from_state_dict(state, compute_dtype: torch.dtype = torch.bfloat16) -> CharLM:
    """A ``CharLM`` with the hyper-parameters a checkpoint's ``model_state``
    implies, its parameters loaded: vocabulary and embedding width from
    ``embedding.weight``, the hidden size from ``lstm.weight_hh_l0``, the
    layers from the key count; DDP's ``module.`` prefix is accepted."""
    from ..train.checkpoint import adapt_state_dict_keys
    plain = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    for k in ("embedding.weight", "lstm.weight_hh_l0", "fc.weight"):
        if k not in plain:
            raise KeyError(f"not a char-LM state: {k} missing")
    vocab, embed = (int(n) for n in plain["embedding.weight"].shape)
    hidden = int(plain["lstm.weight_hh_l0"].shape[1])
    layers = sum(1 for k in plain if k.startswith("lstm.weight_hh_l") and not k.endswith("_reverse"))
    model = CharLM(vocab, embed, hidden, layers, compute_dtype=compute_dtype)
    model.load_state_dict(adapt_state_dict_keys(dict(state), model))
    return model


class BiLSTMEncoder(nn.Module):
    """Stacked bidirectional LSTM with a per-timestep linear head."""

    def __init__(self, input_dim: int, hidden_dim: int, num_layers: int, output_dim: int,
                 compute_dtype: torch.dtype = torch.float16):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.lstm = LSTM(input_dim, hidden_dim, num_layers, batch_first=False, bidirectional=True)
        self.fc = nn.Linear(2 * hidden_dim, output_dim)

    def forward(self, x: Tensor) -> Tensor:
        """x [T, B, I] -> [T, B, output_dim]."""
        cdt = self.compute_dtype if x.is_cuda else torch.float32
        out, _ = self.lstm(x.to(cdt))
        return linear(out, self.fc.weight, self.fc.bias)
