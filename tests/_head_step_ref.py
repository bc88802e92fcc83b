"""fp64 reference of the fused motion training step's contract
(lstm_head_train_step in csrc/bindings.cpp).  Plain torch, no extension
import, on top of tests/_small_ref.py: tests/test_gpu_head_step.py checks this
file against fp64 torch.nn.LSTM / nn.GRU + nn.Linear + cross_entropy autograd
on the CPU and the step's five kernel paths against this file on the GPU.

The contract.  x [N, T, I] is the table of sequences (already widened to fp32
or fp64 when the kernels read bf16); row b of the batch is x[idx[b]] with the
label labels[idx[b]], or x[b] / labels[b] without idx.  The stack starts from
zero state; the loss is the mean cross-entropy of the head's logits on the top
layer's h_T,

    z = h_T head_w^T + head_b,   loss = mean_b (lse(z_b) - z_b[y_b]),
    d = (softmax(z) - onehot(y)) / B,   dh_T = d head_w,
    dhead_w = d^T h_T,   dhead_b = sum_b d.

``flat`` is the gradient in the model's parameter order: per layer w_ih, w_hh,
b_ih, b_hh (both bias slots hold the same sum of gate gradients), then head_w
[C, H], then head_b [C] when the head has one.  The weights arrive in nn order;
for the GRU (cell 1) that is nn.GRU's 3H layout (r, z, n), which this file
packs into the kernels' four row blocks itself (_small_ref.py's docstring) and
unpacks again, so ``flat`` is what grad_colmap produces and none of the packed
zero blocks appears in it.  ``stats`` = [mean loss, B, n_correct]; the predicted
class is the LOWEST index among equal largest logits (torch.argmax on the CPU,
tests/test_gpu_sw_infer.py::test_ties_take_the_lowest_class).

Error budgets.  Every bound below is evaluated on the reference's own fp64
h / act: the step returns no saved rows to force with, so the reference runs
free, and the CPU test test_fp32_reference_run_stays_in_budget shows at every
GPU case's inputs that a plain fp32 run of this file meets them.

  recurrent part of flat   _small_ref.param_grads, unchanged: element (r, k)
      sum_{b,t} (2e-5 + 1e-4 |dg[r]|) |in[k]| + B T 2^-23 sum_{b,t} |dg[r]| |in[k]|

  logits   every h_T[k] may carry the per-element bound 2e-5 + 1e-4 |h_k|, and
      an fp32 sum of H products and the bias adds H + 1 roundings of at most
      2^-24 of the sum of magnitudes:
          ez[b, c] = sum_k |w_ck| (2e-5 + 1e-4 |h_bk|) + (H + 1) 2^-24 sum_k |w_ck h_bk|

  loss   log-softmax is 2-Lipschitz in the max norm (lse is 1-Lipschitz, so is
      the picked logit), so row b's loss moves by at most 2 max_c ez[b, c].  Its
      fp32 evaluation adds the roundings of m + log(se) and of the subtraction
      of z_y, 2^-23 (max_c |z| + log C), and C + 4 ulps of 1 for exp, the sum of
      C terms, log and 1 / B; the fp32 sum over B rows adds B 2^-23 of the mean:
          eloss = mean_b [2 max_c ez + 2^-23 (max_c |z| + log C) + (C + 4) 2^-24] + B 2^-23 mean_b |loss_b|

  d   |log p_c| moves by at most 2 ezmax_b = 2 max_c ez[b, c], so p_c by
      p_c expm1(2 ezmax_b); exp, the sum, the reciprocal, the subtraction of the
      one-hot and the division by B add (C + 8) ulps:
          ed[b, c] = (p_c expm1(2 ezmax_b) + (C + 8) 2^-24 (p_c + onehot)) / B

  head weight   a sum over B of products d h, each over B through d:
          sum_b (ed |h| + |d| eh + ed eh) + B 2^-23 sum_b |d h|,   eh = 2e-5 + 1e-4 |h|
  head bias     sum_b ed + B 2^-23 sum_b |d|

The gate gradients' own bound already stands for whatever reaches them from
dh_T: with |dh_T| of order 1 / B its absolute term 2e-5 dominates.
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

import _small_ref as R

F64 = torch.float64


def pack_gru(ws: Sequence[Tensor], NL: int, H: int) -> List[Tensor]:
    """nn.GRU's (w_ih, w_hh, b_ih, b_hh) per layer -> the four row blocks
    (r, z, n_x, n_h) of _small_ref.py's docstring."""
    out = []
    for l in range(NL):
        w_ih, w_hh, b_ih, b_hh = ws[4 * l:4 * l + 4]
        zi, zh, zb = w_ih.new_zeros(H, w_ih.shape[1]), w_hh.new_zeros(H, H), b_ih.new_zeros(H)
        out += [torch.cat([w_ih, zi]), torch.cat([w_hh[:2 * H], zh, w_hh[2 * H:]]),
                torch.cat([b_ih, zb]), torch.cat([b_hh[:2 * H], zb, b_hh[2 * H:]])]
    return out


def unpack_gru_index(H: int, in_dims: Sequence[int]) -> Tensor:
    """Indices into the packed flat gradient, in nn.GRU's parameter order."""
    idx, off = [], 0
    ih_rows = torch.arange(3 * H)
    hh_rows = torch.cat([torch.arange(2 * H), torch.arange(3 * H, 4 * H)])
    for Il in in_dims:
        idx.append(off + (ih_rows[:, None] * Il + torch.arange(Il)[None, :]).reshape(-1))
        off += 4 * H * Il
        idx.append(off + (hh_rows[:, None] * H + torch.arange(H)[None, :]).reshape(-1))
        off += 4 * H * H
        idx.append(off + ih_rows)
        off += 4 * H
        idx.append(off + hh_rows)
        off += 4 * H
    return torch.cat(idx)


def gather(x: Tensor, idx: Optional[Tensor], labels: Tensor) -> Tuple[Tensor, Tensor]:
    if idx is None:
        return x, labels
    return x.index_select(0, idx), labels.index_select(0, idx)


def lowest_argmax(z: Tensor) -> Tensor:
    C = z.shape[1]
    cls = torch.arange(C, device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, cls, torch.full_like(cls, C)).min(1).values


def step(x: Tensor, idx: Optional[Tensor], labels: Tensor, ws: Sequence[Tensor], head_w: Tensor,
         head_b: Optional[Tensor], cell: int, dtype=F64) -> Dict[str, Tensor]:
    """flat, budget (per element of flat), stats [3], loss_bound (scalar), and
    for the tests: logits [B, C], ez (the logit bound, [B, C]), offsets (name ->
    (start, end) in flat)."""
    H = head_w.shape[1]
    C = head_w.shape[0]
    NL = len(ws) // 4
    xb, y = gather(x, idx, labels)
    xb = xb.to(dtype)
    B, T, _ = xb.shape
    ws = [w.to(dtype) for w in ws]
    w4 = pack_gru(ws, NL, H) if cell == 1 else list(ws)
    hw = head_w.to(dtype)
    hseq, act, hn, _ = R.forward(xb, w4, None, None, H, NL, cell, dtype=dtype)
    h = hn[NL - 1]                                        # [B, H]
    # one product at a time, in the order of k: two identical rows of the head
    # then give the same bits on every machine (a BLAS call need not)
    z = h.new_zeros(B, C)
    for k in range(H):
        z = z + h[:, k, None] * hw[None, :, k]
    if head_b is not None:
        z = z + head_b.to(dtype)
    lse = torch.logsumexp(z, 1)
    onehot = torch.nn.functional.one_hot(y, C).to(dtype)
    row_loss = lse - (z * onehot).sum(1)
    p = torch.exp(z - lse[:, None])
    d = (p - onehot) / B
    dhn = hseq.new_zeros(NL, B, H)
    dhn[NL - 1] = d @ hw
    dparams, budget, _, _, _ = R.backward(xb, w4, None, None, hseq, act, None, dhn, None, H, NL, cell, dtype=dtype)
    if cell == 1:
        sel = unpack_gru_index(H, [int(w4[4 * l].shape[1]) for l in range(NL)]).to(dparams.device)
        dparams, budget = dparams.index_select(0, sel), budget.index_select(0, sel)

    # ---- head budgets (module docstring)
    ha, wa = h.abs(), hw.abs()
    eh = R.ATOL + R.RTOL * ha
    ez = eh @ wa.t() + (H + 1) * 2.0 ** -24 * (ha @ wa.t())
    ezmax = ez.max(1).values
    loss_bound = (2 * ezmax + 2.0 ** -23 * (z.abs().max(1).values + math.log(C)) + (C + 4) * 2.0 ** -24).mean() \
        + B * 2.0 ** -23 * row_loss.abs().mean()
    ed = (p * torch.expm1(2 * ezmax)[:, None] + (C + 8) * 2.0 ** -24 * (p + onehot)) / B
    da = d.abs()
    b_hw = ed.t() @ ha + da.t() @ eh + ed.t() @ eh + B * 2.0 ** -23 * (da.t() @ ha)
    grads, budgets = [dparams, (d.t() @ h).reshape(-1)], [budget, b_hw.reshape(-1)]
    if head_b is not None:
        grads.append(d.sum(0))
        budgets.append(ed.sum(0) + B * 2.0 ** -23 * da.sum(0))
    correct = (lowest_argmax(z) == y).sum()
    stats = torch.stack([row_loss.mean(), row_loss.new_tensor(float(B)), correct.to(dtype)])

    offsets, off = {}, 0
    for l in range(NL):
        for k, name in enumerate(("w_ih", "w_hh", "b_ih", "b_hh")):
            n = ws[4 * l + k].numel()
            offsets[f"{name}_l{l}"] = (off, off + n)
            off += n
    offsets["head_w"] = (off, off + C * H)
    off += C * H
    if head_b is not None:
        offsets["head_b"] = (off, off + C)
    return dict(flat=torch.cat(grads), budget=torch.cat(budgets), stats=stats, loss_bound=loss_bound, logits=z, ez=ez,
                offsets=offsets)


def top2_margin(z: Tensor) -> Tensor:
    """Per row the gap between the largest logit and the largest one that
    differs from it (inf when all are equal): below it a tie or a flip of the
    predicted class is possible."""
    top = z.max(1, keepdim=True).values
    rest = torch.where(z == top, torch.full_like(z, -math.inf), z).max(1).values
    return top[:, 0] - rest


def adam_step(param: Tensor, grad: Tensor, m: Tensor, v: Tensor, lr: float, b1: float, b2: float, eps: float,
              wd: float, step: float, decoupled: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """One plain fp64 Adam / AdamW step (torch.optim semantics) -> (p, m, v).
    The scalars are rounded to fp32 first, as the native launch receives them
    (tests/test_gpu_adam.py adam_ref, whose fp64 form is torch.optim.Adam)."""
    def r(s):
        return float(torch.tensor(s, dtype=torch.float32))
    bc1, bc2_sqrt = r(1.0 - b1 ** step), r(math.sqrt(1.0 - b2 ** step))
    lr, b1, b2, eps, wd = r(lr), r(b1), r(b2), r(eps), r(wd)
    p, g, m, v = param.double(), grad.double(), m.double(), v.double()
    if wd != 0.0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    return p - (lr / bc1) * (m / (v.sqrt() / bc2_sqrt + eps)), m, v
