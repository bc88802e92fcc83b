"""GRU stack operator: fused HIP kernels for small hidden sizes (fp32), the MFMA
step kernels for 16-bit inputs with H % 64 == 0 (ops/gru_large.py), ATen otherwise.

New capability (BASELINE.json names an "LSTM/GRU cell"; the reference itself
only uses nn.LSTM).  Gate order and parameters follow nn.GRU
(r, z, n; n = tanh(W_in x + b_in + r * (W_hn h + b_hn))).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _ext
from .lstm import GRU, run_small_stack, small_plan


def gru_reference(x: Tensor, weights: Sequence[Optional[Tensor]], h0: Optional[Tensor], hidden: int,
                  num_layers: int, batch_first: bool, dropout: float = 0.0,
                  training: bool = False) -> Tuple[Tensor, Tensor]:
    has_bias = weights[2] is not None
    flat = [w for w in weights if w is not None]
    if h0 is None:
        b = x.shape[0] if batch_first else x.shape[1]
        h0 = x.new_zeros(num_layers, b, hidden)
    out, hn = torch._VF.gru(x, h0, flat, has_bias, num_layers, dropout, training, False, batch_first)
    return out, hn


def gru_forward(x: Tensor, weights: Sequence[Optional[Tensor]], h0: Optional[Tensor] = None, *,
                hidden: int, num_layers: int, batch_first: bool = False, dropout: float = 0.0,
                training: bool = False) -> Tuple[Tensor, Tensor]:
    drop = dropout if training else 0.0
    plan = small_plan(x, hidden, num_layers, cell="gru", per_layer=drop > 0, batch_first=batch_first)
    if plan is not None:
        out, hn, _ = run_small_stack(GRU, x, weights, h0, None, plan, hidden=hidden, batch_first=batch_first,
                                     drop=drop)
        return out, hn
    from . import gru_large
    if gru_large.supported(x, hidden):
        return gru_large.gru_large_forward(x, weights, h0, hidden=hidden, num_layers=num_layers,
                                           batch_first=batch_first, dropout=dropout, training=training)
    _ext.fallback(f"GRU(H={hidden}, I={x.shape[-1]}, layers={num_layers}, {x.dtype})", x.device)
    return gru_reference(x, weights, h0, hidden, num_layers, batch_first, dropout, training)
