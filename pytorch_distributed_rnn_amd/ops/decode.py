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
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .. import _ext
from . import shadow as _sh
from .lstm_large import _DTYPE_CODE, _bias_cat, shadow

__all__ = ["gumbel_noise", "keep_threshold", "token_logprobs", "check_filters", "sample", "supported", "alloc_buffers",
           "decode", "reference", "MAX_STREAMS"]

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


def supported(B: int, H: int, E: int, V: int, L: int, dtype: torch.dtype, device) -> bool:
    """The fused decode kernels run this shape on ``device``."""
    device = torch.device(device)
    if device.type != "cuda" or dtype not in _DTYPE_CODE:
        return False
    mod = _ext.native(device)
    if mod is None:
        return False
    if not hasattr(mod, "lstm_decode"):
        raise RuntimeError("the native extension has no lstm_decode: rebuild it (python -m pytorch_distributed_rnn_amd._build)")
    return bool(mod.lstm_decode_supported(B, H, E, V, L, _DTYPE_CODE[dtype]))


def alloc_buffers(L: int, B: int, H: int, V: int, N: int, cdt: torch.dtype, device,
                  return_logits: bool = False, return_threshold: bool = False,
                  return_logprobs: bool = False) -> Dict[str, Optional[Tensor]]:
    """The buffers one ``decode`` call works in: ``h`` [2, L, B, H] (16-bit; the
    state entering position p in slot p & 1), ``c`` [L, B, H] fp32 (in place),
    ``scratch`` [B, V] fp32 (the latest logits), ``tokens`` [B, N] int64 and
    ``logits`` [B, N, V], ``threshold`` [B, N], ``logprobs`` [B, N] fp32 or
    None."""
    f32 = dict(device=device, dtype=torch.float32)
    return {"h": torch.empty(2, L, B, H, device=device, dtype=cdt), "c": torch.empty(L, B, H, **f32),
            "scratch": torch.empty(B, V, **f32), "tokens": torch.empty(B, N, device=device, dtype=torch.int64),
            "logits": torch.empty(B, N, V, **f32) if return_logits else None,
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
    dev = emb_w.device
    mod = _ext.native(dev)
    V, E = emb_w.shape
    H = fc_w.shape[1]
    L = len(lstm_weights) // 4
    B, N = first.shape[0], int(num_tokens)
    if mod is None or not supported(B, H, E, V, L, cdt, dev):
        raise RuntimeError(f"lstm_decode does not cover B={B} H={H} E={E} V={V} L={L} {cdt} on {dev}")
    if N < 1:
        raise ValueError("num_tokens must be at least 1")
    check_filters(top_k, top_p)
    with torch.no_grad():
        w_ih = [shadow(lstm_weights[4 * l], "i", cdt, H) for l in range(L)]
        w_hh = [shadow(lstm_weights[4 * l + 1], "i", cdt, H) for l in range(L)]
        bias = [_bias_cat(list(lstm_weights[4 * l:4 * l + 4]), 1, H, dev) for l in range(L)]
        emb16, fc16 = _sh.cast(emb_w, cdt), _sh.cast(fc_w, cdt)
        if bufs is None:
            bufs = alloc_buffers(L, B, H, V, N, cdt, dev, return_logits, return_threshold, return_logprobs)
        h, c = bufs["h"], bufs["c"]
        h[0].copy_(h0) if h0 is not None else h[0].zero_()
        c.copy_(c0) if c0 is not None else c.zero_()
        mod.lstm_decode(emb16, w_ih, w_hh, bias, fc16, fc_b.detach().float() if fc_b is not None else None, h, c,
                        bufs["scratch"], first.to(dev, torch.int64).contiguous(),
                        forced.to(dev, torch.int64).contiguous() if forced is not None else None, bufs["tokens"],
                        bufs["logits"] if return_logits else None, float(temperature), int(seed) & _M32,
                        int(stream0) & _M32, int(pos0) & _M32, top_k=min(int(top_k), V), top_p=float(top_p),
                        threshold=bufs["threshold"] if return_threshold else None,
                        logprobs=bufs["logprobs"] if return_logprobs else None)
    out = (bufs["tokens"], bufs["logits"] if return_logits else None, h[N & 1], c)
    return out + ((bufs["threshold"],) if return_threshold else ()) + ((bufs["logprobs"],) if return_logprobs else ())


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
