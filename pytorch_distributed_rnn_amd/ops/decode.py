"""Char-LM generation: the fused decode kernels' op, the sampling rule's mirror
and the reference path.

``decode`` drives csrc/kernels/lstm_decode.hip: per generated token one launch
per LSTM layer and one for the vocabulary head, all enqueued from C++ in one
call, sampling inside the layer-0 launch of the next position; nothing is read
back until the caller reads the tokens.  ``reference`` is the same generation
as a host loop over a step function (``CharLM.forward`` one token at a time)
and runs anywhere; both sample by the rule below.

Sampling rule (csrc/include/pdrnn/decode_rng.h is the device's copy; the two
agree word for word in ``r`` and ``u``, and in ``g`` to the last bits of
``log``): for stream ``b`` at position ``pos`` and vocabulary entry ``v``

    r = mix(key(seed, b, pos) ^ v)              32-bit counter hash
    u = min(((r >> 8) + 0.5) * 2^-24, 1 - 2^-24)    in fp32
    g = -log(-log(u))
    token = argmax_v(logit_v / temperature + g_v), the lowest index on ties

which draws from ``softmax(logits / temperature)`` (Gumbel-max).  Temperature
0 is greedy: the argmax of the logits, no noise.

Filters (``keep_threshold`` is the mirror; decode_rng.h states the rule once).
A filter is a per-row threshold ``tau`` on the raw logits, and the draw is the
same argmax over ``{v : logit_v >= tau}`` with the same noise:

    top-k   tau_k = the k-th largest logit counted with multiplicity; every
            entry tied with it is kept (0 or >= V: off)
    top-p   over the top-k survivors, w_v = exp(logit_v / T - max): tau_p = the
            largest logit value with sum{w_v : logit_v >= tau_p} >= top_p *
            sum{w_v : logit_v >= tau_k}; boundary ties are kept (>= 1: off)
    tau     max(tau_k, tau_p), the smallest kept logit; -inf with both off

The log-probability of a drawn token is that under the kept, renormalised
distribution: ``logit_tok / T - max - log(sum{w_v : kept})``.  Greedy ignores
both filters, and its log-probability is the argmax's at temperature 1.

Beam search (``beam_select`` is the mirror of one position; ``beam_decode`` the
fused op, ``beam_reference`` the host loop; decode_rng.h states the rule once).
A launch holds G groups (prompts) of W beams, G * W <= 16; stream ``s = g * W +
j`` is beam j of group g.

    start   the W streams of a group enter position 0 with the prompt's state
            and last token; cum[0] = 0, cum[j > 0] = -inf, done = false
    score   from the position's fp32 logits: m = max_v l[s, v], lp_s(v) =
            (l[s, v] - m) - log(sum_v exp(l[s, v] - m)) in fp32 in that order;
            a live stream's candidates are every v at cum_s + lp_s(v), a done
            stream's only one is v = stop at cum_s with log-prob 0
    select  per group the W best candidates become the new beams in rank
            order: score descending, then source beam j, then v, ascending;
            -inf is an ordinary value, a NaN score ranks (and is kept) as -inf
    slot i  parent[i] = j, token[i] = v, cum[i] = the score, done[i] = done_j
            or v == stop; at the next position it reads token[i]'s embedding
            row and, in every layer, the h and c of slot parent[i]
    end     after N positions the parents are traced back into hypotheses
            [G, W, N] in final rank order; a length counts up to and including
            the first stop, later tokens are stop with log-prob 0; finished
            beams keep running through the LSTM on stop tokens

``length_penalty`` a re-ranks the final W, stably, by cum / length^a
(``beam_finish``): at the end only, on the device.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .. import _ext
from . import shadow as _sh
from .lstm_large import _DTYPE_CODE, _bias_cat, shadow

__all__ = ["gumbel_noise", "keep_threshold", "token_logprobs", "check_filters", "sample", "supported", "alloc_buffers",
           "decode", "reference", "MAX_STREAMS", "check_beam", "beam_start", "beam_select", "beam_backtrace",
           "stop_lengths", "beam_finish", "beam_supported", "alloc_beam_buffers", "beam_decode", "beam_reference"]

MAX_STREAMS = 16  # streams per launch: the 16-wide side of the MFMA tile
_M32 = 0xFFFFFFFF


def _mix(x: Tensor) -> Tensor:
    """decode_mix on uint32 values held in int64 (products wrap mod 2^64: the
    low 32 bits are the 32-bit product's)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _uniform_words(seed: int, b: Tensor, pos: Tensor, V: int) -> Tensor:
    """r of the rule above, [len(pos), len(b), V] int64 in [0, 2^32)."""
    h = _mix(torch.full_like(b, (int(seed) + 0x9E3779B9) & _M32))
    h = _mix(h ^ ((b & _M32) * 0x85EBCA6B & _M32))
    h = _mix(h[None, :] ^ ((pos & _M32) * 0xC2B2AE35 & _M32)[:, None])
    v = torch.arange(V, device=b.device, dtype=torch.int64)
    return _mix(h[:, :, None] ^ v)


def gumbel_noise(seed: int, b: Union[int, Tensor, Sequence[int]], pos: Union[int, Tensor, Sequence[int]], V: int,
                 device=None) -> Tensor:
    """The Gumbel noise the decode kernels add to stream ``b``'s logits at
    position ``pos``: fp32 [V] for an int ``b``, [len(b), V] for several
    streams, with a leading [len(pos)] for several positions."""
    one_b, one_p = isinstance(b, int), isinstance(pos, int)
    bt = torch.as_tensor([b] if one_b else b, dtype=torch.int64, device=device)
    pt = torch.as_tensor([pos] if one_p else pos, dtype=torch.int64, device=bt.device)
    r = _uniform_words(seed, bt, pt, V)
    u = ((r >> 8).to(torch.float32) + 0.5) * 5.9604644775390625e-08
    u = torch.clamp(u, max=0.99999994)
    g = -torch.log(-torch.log(u))
    g = g[:, 0] if one_b else g
    return g[0] if one_p else g


def first_argmax(x: Tensor) -> Tensor:
    """argmax over the last dimension, the lowest index on ties (torch.argmax
    leaves the choice open on the GPU)."""
    V = x.shape[-1]
    idx = torch.arange(V, device=x.device).expand_as(x)
    top = x.max(dim=-1, keepdim=True).values
    return torch.where(x == top, idx, V).min(dim=-1).values.clamp_(max=V - 1)


def check_filters(top_k: int, top_p: float) -> None:
    """ValueError unless top_k >= 0 and 0 < top_p <= 1."""
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0: off), not {top_k}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1] (1: off), not {top_p}")


def _filters_on(V: int, temperature: float, top_k: int, top_p: float) -> bool:
    return temperature != 0 and (0 < top_k < V or top_p < 1)


def keep_threshold(logits: Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0) -> Tensor:
    """tau [...] of the filter rule above for logits [..., V], in the logits'
    dtype (fp32: the reference path's; fp64: a test's yardstick), on their
    device: entry v is kept iff ``logits[..., v] >= tau``."""
    check_filters(top_k, top_p)
    V = logits.shape[-1]
    tau = logits.new_full(logits.shape[:-1], float("-inf"))
    if not _filters_on(V, temperature, top_k, top_p):
        return tau
    top, _ = logits.sort(dim=-1, descending=True)
    if 0 < top_k < V:
        tau = top[..., top_k - 1].clone()
    if top_p < 1:
        y = top / torch.tensor(temperature, dtype=logits.dtype, device=logits.device)
        w = torch.exp(y - y[..., :1])
        w = torch.where(top >= tau[..., None], w, torch.zeros_like(w))
        mass = w.cumsum(dim=-1)
        # the mass at or above a VALUE is the running sum at the last entry of its run of ties:
        # the nearest run end to the right (the running sums do not decrease)
        end = torch.ones_like(top, dtype=torch.bool)
        end[..., :-1] = top[..., :-1] != top[..., 1:]
        at_value = torch.where(end, mass, torch.full_like(mass, float("inf"))).flip(-1).cummin(dim=-1).values.flip(-1)
        enough = (at_value >= top_p * mass[..., -1:]) & (top >= tau[..., None])
        tau = torch.where(enough, top, torch.full_like(top, float("-inf"))).max(dim=-1).values
    return tau


def token_logprobs(logits: Tensor, tokens: Tensor, temperature: float, tau: Optional[Tensor] = None) -> Tensor:
    """Log-probabilities [...] of ``tokens`` [...] under the kept distribution
    of logits [..., V] (``tau`` [...] from ``keep_threshold``; None: nothing
    filtered), in the logits' dtype.  Temperature 0: the unfiltered
    distribution at temperature 1."""
    if temperature == 0:
        temperature, tau = 1.0, None
    y = logits / torch.tensor(temperature, dtype=logits.dtype, device=logits.device)
    top = y.max(dim=-1, keepdim=True).values
    w = torch.exp(y - top)
    if tau is not None:
        w = torch.where(logits >= tau[..., None], w, torch.zeros_like(w))
    return y.gather(-1, tokens[..., None])[..., 0] - top[..., 0] - torch.log(w.sum(dim=-1))


def sample(logits: Tensor, temperature: float, seed: int, streams: Tensor, pos: int,
           noise: Optional[Tensor] = None, top_k: int = 0, top_p: float = 1.0,
           tau: Optional[Tensor] = None) -> Tensor:
    """Tokens [B] from fp32 logits [B, V] by the rule above; ``streams`` [B]:
    each row's global stream index; ``noise``: gumbel_noise(seed, streams,
    pos, V) when the caller has it already; ``tau`` [B]: keep_threshold(logits,
    temperature, top_k, top_p) likewise."""
    logits = logits.float()
    if temperature == 0:
        return first_argmax(logits)
    if noise is None:
        noise = gumbel_noise(seed, streams.to(logits.device), pos, logits.shape[-1], device=logits.device)
    y = logits / torch.tensor(temperature, dtype=torch.float32, device=logits.device) + noise
    if tau is None and _filters_on(logits.shape[-1], temperature, top_k, top_p):
        tau = keep_threshold(logits, temperature, top_k, top_p)
    if tau is not None:
        y = torch.where(logits >= tau[:, None], y, torch.full_like(y, float("-inf")))
    return first_argmax(y)


def _covered(op: str, dtype: torch.dtype, device, *shape: int) -> bool:
    """The extension on ``device`` has ``op``, and ``<op>_supported`` covers ``shape`` in ``dtype``."""
    device = torch.device(device)
    mod = _ext.native(device) if device.type == "cuda" and dtype in _DTYPE_CODE else None
    if mod is None:
        return False
    if not hasattr(mod, op):
        raise RuntimeError(f"the native extension has no {op}: rebuild it (python -m pytorch_distributed_rnn_amd._build)")
    return bool(getattr(mod, op + "_supported")(*shape, _DTYPE_CODE[dtype]))


def supported(B: int, H: int, E: int, V: int, L: int, dtype: torch.dtype, device) -> bool:
    """The fused decode kernels run this shape on ``device``."""
    return _covered("lstm_decode", dtype, device, B, H, E, V, L)


def _stack_dims(emb_w: Tensor, lstm_weights: Sequence[Tensor], fc_w: Tensor) -> tuple:
    """(the device, its extension or None, V, E, H, L) of a stack."""
    return (emb_w.device, _ext.native(emb_w.device), *emb_w.shape, fc_w.shape[1], len(lstm_weights) // 4)


def _stack_operands(emb_w: Tensor, lstm_weights: Sequence[Tensor], fc_w: Tensor, fc_b: Optional[Tensor], cdt) -> tuple:
    """Both ops' leading arguments: emb, w_ih / w_hh / b_ih + b_hh per layer, fc_w, fc_b; the weights in
    ``cdt`` from the shadow registry, the biases in fp32."""
    H, L = fc_w.shape[1], len(lstm_weights) // 4
    w_ih = [shadow(lstm_weights[4 * l], "i", cdt, H) for l in range(L)]
    w_hh = [shadow(lstm_weights[4 * l + 1], "i", cdt, H) for l in range(L)]
    bias = [_bias_cat(list(lstm_weights[4 * l:4 * l + 4]), 1, H, emb_w.device) for l in range(L)]
    return (_sh.cast(emb_w, cdt), w_ih, w_hh, bias, _sh.cast(fc_w, cdt), fc_b.detach().float() if fc_b is not None else None)


def _alloc_stack(L: int, B: int, H: int, V: int, N: int, cdt, device, return_logits: bool) -> Dict[str, Optional[Tensor]]:
    """What both ops work in: ``h``, ``c``, ``scratch`` and ``logits`` of ``alloc_buffers``."""
    f32 = dict(device=device, dtype=torch.float32)
    return {"h": torch.empty(2, L, B, H, device=device, dtype=cdt), "c": torch.empty(L, B, H, **f32),
            "scratch": torch.empty(B, V, **f32), "logits": torch.empty(B, N, V, **f32) if return_logits else None}


def alloc_buffers(L: int, B: int, H: int, V: int, N: int, cdt: torch.dtype, device,
                  return_logits: bool = False, return_threshold: bool = False,
                  return_logprobs: bool = False) -> Dict[str, Optional[Tensor]]:
    """The buffers one ``decode`` call works in: ``h`` [2, L, B, H] (16-bit; the
    state entering position p in slot p & 1), ``c`` [L, B, H] fp32 (in place),
    ``scratch`` [B, V] fp32 (the latest logits), ``tokens`` [B, N] int64 and
    ``logits`` [B, N, V], ``threshold`` [B, N], ``logprobs`` [B, N] fp32 or
    None."""
    f32 = dict(device=device, dtype=torch.float32)
    return {**_alloc_stack(L, B, H, V, N, cdt, device, return_logits), "tokens": torch.empty(B, N, device=device, dtype=torch.int64),
            "threshold": torch.empty(B, N, **f32) if return_threshold else None,
            "logprobs": torch.empty(B, N, **f32) if return_logprobs else None}


def decode(emb_w: Tensor, lstm_weights: Sequence[Tensor], fc_w: Tensor, fc_b: Optional[Tensor], cdt: torch.dtype,
           h0: Optional[Tensor], c0: Optional[Tensor], first: Tensor, num_tokens: int, *, temperature: float = 1.0,
           seed: int = 0, stream0: int = 0, pos0: int = 0, forced: Optional[Tensor] = None,
           return_logits: bool = False, bufs: Optional[Dict[str, Optional[Tensor]]] = None, top_k: int = 0,
           top_p: float = 1.0, return_threshold: bool = False, return_logprobs: bool = False):
    """``num_tokens`` positions on the fused kernels for B <= 16 streams.

    emb_w [V, E], lstm_weights (w_ih, w_hh, b_ih, b_hh per layer), fc_w [V, H],
    fc_b: the fp32 masters; their 16-bit copies come from the shadow registry,
    so a call after an optimizer step reads the new weights.  h0 / c0
    [L, B, H] or None (zeros); first [B]: position 0's input tokens; forced
    [B, num_tokens]: every position's input instead.  ``bufs``: caller-made
    buffers (``alloc_buffers``).  ``top_k`` / ``top_p``: the filters of the
    rule above, found inside the layer-0 launch.  Returns (tokens [B, N],
    logits [B, N, V] or None, h [L, B, H] in ``cdt``, c [L, B, H] fp32), then
    the thresholds [B, N] and the tokens' log-probabilities [B, N] (fp32), each
    only when asked for: views of the buffers."""
    dev, mod, V, E, H, L = _stack_dims(emb_w, lstm_weights, fc_w)
    B, N = first.shape[0], int(num_tokens)
    if mod is None or not supported(B, H, E, V, L, cdt, dev):
        raise RuntimeError(f"lstm_decode does not cover B={B} H={H} E={E} V={V} L={L} {cdt} on {dev}")
    if N < 1:
        raise ValueError("num_tokens must be at least 1")
    check_filters(top_k, top_p)
    with torch.no_grad():
        stack = _stack_operands(emb_w, lstm_weights, fc_w, fc_b, cdt)
        if bufs is None:
            bufs = alloc_buffers(L, B, H, V, N, cdt, dev, return_logits, return_threshold, return_logprobs)
        h, c = bufs["h"], bufs["c"]
        h[0].copy_(h0) if h0 is not None else h[0].zero_()
        c.copy_(c0) if c0 is not None else c.zero_()
        mod.lstm_decode(*stack, h, c, bufs["scratch"], first.to(dev, torch.int64).contiguous(),
                        forced.to(dev, torch.int64).contiguous() if forced is not None else None, bufs["tokens"],
                        bufs["logits"] if return_logits else None, float(temperature), int(seed) & _M32,
                        int(stream0) & _M32, int(pos0) & _M32, top_k=min(int(top_k), V), top_p=float(top_p),
                        threshold=bufs["threshold"] if return_threshold else None,
                        logprobs=bufs["logprobs"] if return_logprobs else None)
    out = (bufs["tokens"], bufs["logits"] if return_logits else None, h[N & 1], c)
    return out + ((bufs["threshold"],) if return_threshold else ()) + ((bufs["logprobs"],) if return_logprobs else ())


def check_beam(width: int, stop: Optional[int], V: int, num_tokens: int = 1, groups: int = 1) -> None:
    """ValueError unless 1 <= width <= 16, groups * width <= 16, stop is None
    or a token of the vocabulary, and num_tokens >= 1."""
    if int(width) != width or not 1 <= width <= MAX_STREAMS:
        raise ValueError(f"beam_width must be an integer in [1, {MAX_STREAMS}], not {width}")
    if groups < 1 or groups * width > MAX_STREAMS:
        raise ValueError(f"{groups} groups of {width} beams do not fit a launch's {MAX_STREAMS} streams")
    if stop is not None and not 0 <= int(stop) < V:
        raise ValueError(f"stop token {stop} is outside the vocabulary")
    if int(num_tokens) < 1:
        raise ValueError("num_tokens must be at least 1")


def beam_start(groups: int, width: int, device=None, dtype: torch.dtype = torch.float32) -> Tensor:
    """The scores [groups * width] entering position 0: 0 for a group's beam
    0, -inf for its copies."""
    cum = torch.full((groups, width), float("-inf"), device=device, dtype=dtype)
    cum[:, 0] = 0
    return cum.reshape(-1)


def beam_select(logits: Tensor, cum: Tensor, done: Tensor, width: int, stop: Optional[int] = None):
    """One position of the beam rule for logits [S, V] (fp32: the reference
    path's; fp64: a test's yardstick), scores ``cum`` [S] and ``done`` [S]
    (bool), S = G * width streams, on their device -> (parent [S] int64 stream
    indices, token [S] int64, cum [S], done [S] bool, lp [S]) of the new slots.
    A done stream needs ``stop``: that token is its only candidate."""
    S, V = logits.shape
    W = int(width)
    G = S // W
    if G * W != S:
        raise ValueError(f"beam_select: {S} streams are no multiple of the width {W}")
    dt, dev = logits.dtype, logits.device
    cum, done = cum.to(dev, dt).reshape(S, 1), done.to(dev).to(torch.bool).reshape(S, 1)
    ninf = torch.full((), float("-inf"), dtype=dt, device=dev)
    d = logits - logits.max(dim=-1, keepdim=True).values
    lp = d - torch.log(torch.exp(d).sum(dim=-1, keepdim=True))
    lp = torch.where(done, torch.zeros_like(lp), lp)
    cand = cum + lp
    cand = torch.where(torch.isnan(cand), ninf, cand) + 0.0  # (NaN ranks as -inf; -0 + 0 = +0)
    v = torch.arange(V, device=dev)
    absent = done & (v != (-1 if stop is None else int(stop)))[None, :]
    flat, gone = cand.reshape(G, W * V), absent.reshape(G, W * V)
    # (j, v) ascending is the flat order: a stable sort keeps it among equal scores
    by_score = flat.sort(dim=-1, descending=True, stable=True).indices
    present_first = gone.gather(-1, by_score).to(torch.int8).sort(dim=-1, stable=True).indices
    idx = by_score.gather(-1, present_first)[:, :W]
    parent = (idx // V + torch.arange(G, device=dev)[:, None] * W).reshape(S)
    token = (idx % V).reshape(S)
    new_done = done.reshape(S)[parent] | (token == (-1 if stop is None else int(stop)))
    return parent, token, flat.gather(-1, idx).reshape(S), new_done, lp.reshape(G, W * V).gather(-1, idx).reshape(S)


def beam_backtrace(tokens: Tensor, parents: Tensor, lp: Optional[Tensor] = None):
    """Hypotheses [S, N] in final slot order from the per-selection records
    tokens / parents (/ lp) [S, N] -> (hyp, hyp_lp or None)."""
    S, N = tokens.shape
    at = torch.arange(S, device=tokens.device)
    hyp = torch.empty_like(tokens)
    hyp_lp = torch.empty_like(lp) if lp is not None else None
    for q in range(N - 1, -1, -1):
        hyp[:, q] = tokens[at, q]
        if lp is not None:
            hyp_lp[:, q] = lp[at, q]
        at = parents[at, q].to(torch.int64)
    return hyp, hyp_lp


def stop_lengths(tokens: Tensor, stop: Optional[int]) -> Tuple[Tensor, Tensor]:
    """tokens [..., N] -> (lengths [...] int64 up to and including the first ``stop``, N without one;
    past [..., N] bool: the positions after it)."""
    hit = tokens == stop if stop is not None else torch.zeros_like(tokens, dtype=torch.bool)
    before = hit.cumsum(dim=-1) - hit.to(torch.int64)  # the stop tokens before each position
    return (before == 0).sum(dim=-1).to(torch.int64), before > 0


def beam_finish(hyp: Tensor, scores: Tensor, stop: Optional[int], length_penalty: float = 0.0):
    """Lengths and the final order, on the device with no host read: hyp
    [G, W, N], scores [G, W] in rank order -> (order [G, W], lengths [G, W]
    int64, ranked scores [G, W]).  A length counts up to and including the first
    ``stop``; ``length_penalty`` a != 0 re-ranks, stably, by score / length^a."""
    lengths, _ = stop_lengths(hyp, stop)
    order = torch.arange(hyp.shape[1], device=hyp.device).expand(hyp.shape[0], -1)
    if length_penalty:
        scores = scores / lengths.to(scores.dtype) ** float(length_penalty)
        order = torch.where(torch.isnan(scores), torch.full_like(scores, float("-inf")), scores).sort(
            dim=-1, descending=True, stable=True).indices
        scores, lengths = scores.gather(-1, order), lengths.gather(-1, order)
    return order, lengths, scores


def beam_supported(G: int, W: int, H: int, E: int, V: int, L: int, dtype: torch.dtype, device) -> bool:
    """The fused decode kernels run a beam search of G groups of W beams."""
    return _covered("lstm_decode_beam", dtype, device, G, W, H, E, V, L)


def alloc_beam_buffers(L: int, G: int, W: int, H: int, V: int, N: int, cdt: torch.dtype, device,
                       return_logits: bool = False, return_logprobs: bool = False) -> Dict[str, Optional[Tensor]]:
    """The buffers one ``beam_decode`` call works in, S = G * W: ``h``
    [2, L, S, H], ``c`` [L, S, H], ``scratch`` [S, V] as in ``alloc_buffers``;
    ``cum`` [N + 1, S] fp32 and ``done`` [N + 1, S] int32 (row q enters
    position q); ``tokens`` [S, N] int64, ``parents`` [S, N] int32 and ``lp``
    [S, N] fp32 or None per selection; ``logits`` [S, N, V] or None per slot and
    position; ``hyp`` [S, N] int64 and ``hyp_lp`` [S, N] or None: the traced-back
    hypotheses."""
    S = G * W
    f32 = dict(device=device, dtype=torch.float32)
    i64 = dict(device=device, dtype=torch.int64)
    i32 = dict(device=device, dtype=torch.int32)
    return {**_alloc_stack(L, S, H, V, N, cdt, device, return_logits),
            "cum": torch.empty(N + 1, S, **f32), "done": torch.empty(N + 1, S, **i32),
            "tokens": torch.empty(S, N, **i64), "parents": torch.empty(S, N, **i32),
            "lp": torch.empty(S, N, **f32) if return_logprobs else None, "hyp": torch.empty(S, N, **i64),
            "hyp_lp": torch.empty(S, N, **f32) if return_logprobs else None}


def beam_decode(emb_w: Tensor, lstm_weights: Sequence[Tensor], fc_w: Tensor, fc_b: Optional[Tensor], cdt: torch.dtype,
                h0: Optional[Tensor], c0: Optional[Tensor], first: Tensor, num_tokens: int, width: int, *,
                stop: Optional[int] = None, return_logits: bool = False, return_logprobs: bool = False,
                bufs: Optional[Dict[str, Optional[Tensor]]] = None):
    """Beam search over ``num_tokens`` positions on the fused kernels: G =
    len(first) prompts, ``width`` beams each, G * width <= 16.

    The weights as in ``decode`` (16-bit copies from the shadow registry); h0 /
    c0 [L, G, H] or None: each prompt's state, which all its beams start from;
    first [G]: the prompts' last tokens.  ``bufs``: caller-made buffers
    (``alloc_beam_buffers``); they keep every selection's record.  Returns
    (hyp [G, W, N] int64 in rank order, scores [G, W] fp32, hyp_lp [G, W, N] or
    None, h [L, G * W, H] in ``cdt``, c [L, G * W, H] fp32): the state entering
    position N of each hypothesis, the last token not fed, as in ``decode``."""
    dev, mod, V, E, H, L = _stack_dims(emb_w, lstm_weights, fc_w)
    G, N, W = first.shape[0], int(num_tokens), int(width)
    check_beam(width, stop, V, N, G)
    if mod is None or not beam_supported(G, W, H, E, V, L, cdt, dev):
        raise RuntimeError(f"lstm_decode_beam does not cover G={G} W={W} H={H} E={E} V={V} L={L} {cdt} on {dev}")
    with torch.no_grad():
        stack = _stack_operands(emb_w, lstm_weights, fc_w, fc_b, cdt)
        if bufs is None:
            bufs = alloc_beam_buffers(L, G, W, H, V, N, cdt, dev, return_logits, return_logprobs)
        h, c = bufs["h"], bufs["c"]
        h[0].view(L, G, W, H).copy_(h0[:, :, None, :]) if h0 is not None else h[0].zero_()
        c.view(L, G, W, H).copy_(c0[:, :, None, :]) if c0 is not None else c.zero_()
        bufs["cum"][0].copy_(beam_start(G, W, dev))
        bufs["done"][0].zero_()
        mod.lstm_decode_beam(*stack, h, c, bufs["scratch"], first.to(dev, torch.int64).repeat_interleave(W).contiguous(),
                             bufs["cum"], bufs["done"], bufs["tokens"], bufs["parents"],
                             bufs["lp"] if return_logprobs else None, bufs["logits"] if return_logits else None,
                             bufs["hyp"], bufs["hyp_lp"] if return_logprobs else None, G, W,
                             -1 if stop is None else int(stop))
        last = bufs["parents"][:, N - 1].to(torch.int64)
        hn, cn = h[N & 1].index_select(1, last), c.index_select(1, last)
    return (bufs["hyp"].view(G, W, N), bufs["cum"][N].view(G, W),
            bufs["hyp_lp"].view(G, W, N) if return_logprobs else None, hn, cn)


def beam_reference(step: Callable[[Tensor, object], Tuple[Tensor, object]], state, first: Tensor, num_tokens: int,
                   width: int, *, stop: Optional[int] = None, return_logprobs: bool = False,
                   return_trace: bool = False, dtype: torch.dtype = torch.float32):
    """The same search as a host loop: ``step(tokens [S, 1], state) -> (logits
    [S, V], state)`` once per position on S = G * width streams, ``state`` a
    tuple of [layers, streams, H] tensors (or None), then ``beam_select`` in
    ``dtype`` and a gather of the state by the parents.  Returns (hyp
    [G, W, N], scores [G, W], hyp_lp [G, W, N] or None, state) as
    ``beam_decode`` does, then, asked for, the trace: a dict of ``tokens``,
    ``parents``, ``lp`` [S, N], ``cum``, ``done`` [N + 1, S] and ``logits``
    [S, N, V]."""
    G, N, W = first.shape[0], int(num_tokens), int(width)
    dev = first.device
    S = G * W
    src = torch.arange(G, device=dev).repeat_interleave(W)
    with torch.no_grad():
        if state is not None:
            state = tuple(x.index_select(1, src) for x in state)
        tok = first[src]
        cum, done = beam_start(G, W, dev, dtype), torch.zeros(S, dtype=torch.bool, device=dev)
        toks, pars, lps, cums, dones, lgs = [], [], [], [cum], [done], []
        parent = torch.arange(S, device=dev)
        for p in range(N):
            logits, state = step(tok.reshape(S, 1), state)
            logits = logits.to(dtype)
            parent, tok, cum, done, lp = beam_select(logits, cum, done, W, stop)
            toks.append(tok), pars.append(parent), lps.append(lp), cums.append(cum), dones.append(done)
            if return_trace:
                lgs.append(logits)
            if p + 1 < N:
                state = tuple(x.index_select(1, parent) for x in state)
        state = tuple(x.index_select(1, parent) for x in state)
        tokens, parents, lp = torch.stack(toks, 1), torch.stack(pars, 1), torch.stack(lps, 1)
        hyp, hyp_lp = beam_backtrace(tokens, parents, lp if return_logprobs else None)
    out = (hyp.view(G, W, N), cum.view(G, W), hyp_lp.view(G, W, N) if return_logprobs else None, state)
    if return_trace:
        out += ({"tokens": tokens, "parents": parents, "lp": lp, "cum": torch.stack(cums), "done": torch.stack(dones),
                 "logits": torch.stack(lgs, 1)},)
    return out


def reference(step: Callable[[Tensor, object], Tuple[Tensor, object]], state, first: Tensor, num_tokens: int, *,
              temperature: float = 1.0, seed: int = 0, streams: Optional[Tensor] = None, pos0: int = 0,
              forced: Optional[Tensor] = None, return_logits: bool = False, top_k: int = 0, top_p: float = 1.0,
              return_threshold: bool = False, return_logprobs: bool = False):
    """The same generation as a host loop: ``step(tokens [B, 1], state) ->
    (logits [B, V], state)`` once per position, then ``sample`` (with the
    filters through ``keep_threshold``, in fp32).  Returns (tokens [B, N],
    logits [B, N, V] fp32 or None, state), then the thresholds [B, N] and the
    tokens' log-probabilities [B, N], each only when asked for."""
    check_filters(top_k, top_p)
    B = first.shape[0]
    dev = first.device
    streams = torch.arange(B, device=dev) if streams is None else streams.to(dev)
    tokens = torch.empty(B, num_tokens, device=dev, dtype=torch.int64)
    out, taus, lps = [], [], []
    tok = first
    noise, block = None, 64  # the noise of 64 positions at a time: the hash is a dozen small launches
    with torch.no_grad():
        for p in range(num_tokens):
            inp = forced[:, p] if forced is not None else tok
            logits, state = step(inp.reshape(B, 1), state)
            logits = logits.float()
            if temperature != 0 and p % block == 0:
                noise = gumbel_noise(seed, streams, torch.arange(pos0 + p, pos0 + min(p + block, num_tokens), device=dev),
                                     logits.shape[-1], device=dev)
            tau = keep_threshold(logits, temperature, top_k, top_p)
            tok = sample(logits, temperature, seed, streams, pos0 + p, noise[p % block] if noise is not None else None,
                         tau=tau if _filters_on(logits.shape[-1], temperature, top_k, top_p) else None)
            tokens[:, p] = tok
            if return_logits:
                out.append(logits)
            if return_threshold:
                taus.append(tau)
            if return_logprobs:
                lps.append(token_logprobs(logits, tok, temperature, tau))

    def cols(xs):
        return torch.stack(xs, 1) if xs else torch.empty(B, 0, device=dev)

    return ((tokens, torch.stack(out, 1) if return_logits else None, state)
            + ((cols(taus),) if return_threshold else ()) + ((cols(lps),) if return_logprobs else ()))
