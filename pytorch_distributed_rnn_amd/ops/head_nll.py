"""Char-LM evaluation: the fused vocabulary head + log-softmax + NLL op.

``head_nll`` drives csrc/kernels/head_nll.hip: logits = h W^T + b stay in the
fp32 MFMA accumulators from the product to the loss -- never stored, never
rounded to 16 bits -- and one launch returns per row

    row_nll = logsumexp(logits) - logits[label]     (0 where the row is ignored)
    pred    = argmax(logits), the lowest index on ties

and adds ``[sum row_nll, n_valid, n_correct]`` to a three-element fp64
accumulator on the device, so a whole evaluation needs one host read.  A row
is valid on kernels/xent.hip's terms (label != ignore_index and inside the
vocabulary) and correct when it is valid and ``pred == label``.

``reference`` is the same computation in torch (the head in fp32,
``F.cross_entropy(reduction="none")``, a first-index argmax, the three sums in
fp64) and runs anywhere; ``head_nll`` takes it for everything the kernel does
not cover, announced through ``_ext.fallback`` (an error under hip-strict).
No autograd: both run under ``no_grad``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _ext
from . import shadow as _sh
from .decode import first_argmax
from .lstm_large import _DTYPE_CODE

__all__ = ["head_nll", "reference", "supported", "new_accum"]


def new_accum(device) -> Tensor:
    """A zeroed [sum row_nll, n_valid, n_correct] accumulator (fp64 [3])."""
    return torch.zeros(3, dtype=torch.float64, device=device)


def supported(H: int, V: int, dtype: torch.dtype, device) -> bool:
    """The fused kernel runs this head shape on ``device``."""
    device = torch.device(device)
    if device.type != "cuda" or dtype not in _DTYPE_CODE:
        return False
    mod = _ext.native(device)
    if mod is None:
        return False
    if not hasattr(mod, "head_nll"):
        raise RuntimeError("the native extension has no head_nll: rebuild it (python -m pytorch_distributed_rnn_amd._build)")
    return bool(mod.head_nll_supported(H, V, _DTYPE_CODE[dtype]))


def reference(h: Tensor, weight: Tensor, bias: Optional[Tensor], labels: Tensor, ignore_index: int = -100,
              accum: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``head_nll`` in torch: the head in fp32 on ``h`` and ``weight`` as
    given (a 16-bit ``h`` is widened, the fp32 master weight is not rounded)."""
    with torch.no_grad():
        h2 = h.reshape(-1, h.shape[-1]).float()
        labels = labels.reshape(-1).to(h2.device, torch.int64)
        logits = F.linear(h2, weight.detach().float(), bias.detach().float() if bias is not None else None)
        V = logits.shape[-1]
        valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
        safe = torch.where(valid, labels, torch.full_like(labels, ignore_index))
        row_nll = F.cross_entropy(logits, safe, ignore_index=ignore_index, reduction="none")
        pred = first_argmax(logits).to(torch.int32)
        if accum is None:
            accum = new_accum(h2.device)
        accum += torch.stack([row_nll.double().sum(), valid.sum().double(), ((pred == labels) & valid).sum().double()])
    return row_nll, pred, accum


def head_nll(h: Tensor, weight: Tensor, bias: Optional[Tensor], labels: Tensor, ignore_index: int = -100,
             accum: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(row_nll [N] fp32, pred [N] int32, accum [3] fp64) of ``h`` [..., H]
    (rows may be strided: the recurrence's output is read in place) against
    ``labels`` [...].

    ``weight`` [V, H] and ``bias`` [V] are the fp32 masters; the 16-bit weight
    the kernel reads comes from the shadow registry, so a call after an
    optimizer step sees the new weights.  ``accum`` is added to (a new zeroed
    one when None) and returned."""
    dev = h.device
    H = h.shape[-1]
    V = weight.shape[0]
    if not supported(H, V, h.dtype, dev):
        _ext.fallback(f"head_nll (H={H}, V={V}, {h.dtype})", dev)
        return reference(h, weight, bias, labels, ignore_index, accum)
    mod = _ext.native(dev)
    with torch.no_grad():
        h2 = h.detach()
        if h2.dim() != 2:
            h2 = h2.reshape(-1, H)  # (a view where the leading dimensions collapse, else a copy)
        if h2.stride(1) != 1 or h2.stride(0) % 8 or h2.stride(0) < H or h2.data_ptr() % 16:
            h2 = h2.contiguous()
        w16 = _sh.cast(weight, h.dtype)
        b = bias.detach().float() if bias is not None else None
        if accum is None:
            accum = new_accum(dev)
        row_nll, pred = mod.head_nll(h2, w16, b, labels.reshape(-1).to(dev, torch.int64).contiguous(),
                                     int(ignore_index), accum)
    return row_nll, pred, accum
