"""fp64 reference of the fused small-H stack contract (lstm_small_fwd /
lstm_small_bwd in csrc/bindings.cpp, as ops/lstm.py and ops/gru_fused.py call
them).  Plain torch, no extension import: tests/test_gpu_lstm_small_steps.py
checks this file against fp64 torch.nn.LSTM / torch.nn.GRU on the CPU and the
kernels of csrc/kernels/lstm_small.hip against this file on the GPU.

Layouts, as the kernels store them (NL layers, H hidden units, batch-major
whatever the layout of x):
  x       [B, T, I]        here always batch-major, gathered and widened
  w       4 tensors per layer, nn.LSTM order: w_ih [4H, I_l], w_hh [4H, H],
          b_ih [4H] or None, b_hh [4H] or None; I_0 = I, I_l = H above
  h0, c0  [NL, B, H] or None (zeros)
  hseq    [NL, B, T, H]    every layer's h_t
  act     [NL, B, T, 5, H] LSTM: post-activation i, f, g, o, then c_t
                           GRU:  r, z, n_x, n_h, n  (n_x, n_h linear)
  hn, cn  [NL, B, H]       (the GRU has no cn: the kernels leave it unwritten)
  dparams [P]              flat, per layer dw_ih, dw_hh and, when the stack
                           has biases, db_ih, db_hh (stack_layout): both bias
                           slots hold the same sum of gate gradients
cell 0 = LSTM, gate blocks (i, f, g, o).  cell 1 = GRU on the same four row
blocks (r, z, n_x, n_h), packed by ops/gru_fused._pack:
  W_ih4 = [W_ir; W_iz; W_in; 0]   W_hh4 = [W_hr; W_hz; 0; W_hn]
  b_ih4 = [b_ir; b_iz; b_in; 0]   b_hh4 = [b_hr; b_hz; 0; b_hn]
  n = tanh(n_x + r n_h),  h = n + z (h_prev - n).
The gradients of the zero blocks are formed like every other (dg^T in) and
dropped by gru_fused._unpack_index.

forward(..., forced=(hseq, act)) is teacher-forced: step t of layer l is
evaluated on forced hseq[l, t-1], act[l, t-1] (c_{t-1}; the GRU takes h_{t-1}
from hseq) and hseq[l-1, t], so with the kernel's stored tensors there every
step is compared on identical inputs.  Without ``forced`` it runs free (the
inference build stores nothing to force with).

backward() runs free on the given hseq / act (the general kernels return no
per-step gradients to force with) and returns next to dparams an error budget
per element: with the gate gradients dg and the operands ``in`` of a weight
element (r, k), n = B T,

    budget[r, k] = sum_{b,t} (2e-5 + 1e-4 |dg[r]|) |in[k]|  +  n 2^-23 sum_{b,t} |dg[r]| |in[k]|

(biases: in = 1): every product may carry the per-element fp32 bound of its
gate gradient, and an fp32 sum of n terms in any order adds at most n ulps of
the sum of magnitudes.

All functions compute in ``dtype`` (fp64; fp32 gives the plain-torch fp32 run
the long-sequence cases are measured against).
"""
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

ATOL, RTOL = 2e-5, 1e-4


def _cast(t: Optional[Tensor], dtype) -> Optional[Tensor]:
    return None if t is None else t.to(dtype)


def _layer(w: Sequence[Optional[Tensor]], l: int, dtype):
    w_ih, w_hh, b_ih, b_hh = w[4 * l:4 * l + 4]
    b = w_ih.new_zeros(w_ih.shape[0], dtype=dtype)
    for t in (b_ih, b_hh):
        if t is not None:
            b = b + t.to(dtype)
    return w_ih.to(dtype), w_hh.to(dtype), b


def _cell(inp: Tensor, hp: Tensor, cp: Tensor, w_ih: Tensor, w_hh: Tensor, b: Tensor, H: int, cell: int):
    """One step on [..., I_l] / [..., H] operands -> (h, the five saved slots)."""
    z = inp @ w_ih.t() + hp @ w_hh.t() + b
    z0, z1, z2, z3 = z[..., :H], z[..., H:2 * H], z[..., 2 * H:3 * H], z[..., 3 * H:]
    if cell == 0:
        i, f, g, o = torch.sigmoid(z0), torch.sigmoid(z1), torch.tanh(z2), torch.sigmoid(z3)
        c = f * cp + i * g
        return o * torch.tanh(c), (i, f, g, o, c)
    r, zg = torch.sigmoid(z0), torch.sigmoid(z1)
    n = torch.tanh(z2 + r * z3)
    return n + zg * (hp - n), (r, zg, z2, z3, n)


def forward(x: Tensor, w: Sequence[Optional[Tensor]], h0: Optional[Tensor], c0: Optional[Tensor], H: int, NL: int,
            cell: int = 0, forced: Optional[Tuple[Tensor, Tensor]] = None, dtype=torch.float64):
    """hseq, act, hn, cn.  forced = (hseq, act): see the module docstring."""
    x, h0, c0 = x.to(dtype), _cast(h0, dtype), _cast(c0, dtype)
    B, T, _ = x.shape
    zero = x.new_zeros(B, H)
    hseq = x.new_zeros(NL, B, T, H)
    act = x.new_zeros(NL, B, T, 5, H)
    hn, cn = x.new_zeros(NL, B, H), x.new_zeros(NL, B, H)
    if forced is not None:  # no step depends on another: all T at once
        fh, fa = forced[0].to(dtype), forced[1].to(dtype)
        for l in range(NL):
            w_ih, w_hh, b = _layer(w, l, dtype)
            first_h = (h0[l] if h0 is not None else zero)[:, None]
            first_c = (c0[l] if c0 is not None else zero)[:, None]
            hp = torch.cat([first_h, fh[l, :, :-1]], 1)
            cp = torch.cat([first_c, fa[l, :, :-1, 4]], 1)
            h, slots = _cell(x if l == 0 else fh[l - 1], hp, cp, w_ih, w_hh, b, H, cell)
            hseq[l], act[l] = h, torch.stack(slots, 2)
            hn[l], cn[l] = h[:, -1], slots[4][:, -1]
        return hseq, act, hn, cn
    for l in range(NL):
        w_ih, w_hh, b = _layer(w, l, dtype)
        hp = h0[l] if h0 is not None else zero
        cp = c0[l] if c0 is not None else zero
        for t in range(T):
            hp, slots = _cell(x[:, t] if l == 0 else hseq[l - 1, :, t], hp, cp, w_ih, w_hh, b, H, cell)
            cp = slots[4]
            hseq[l, :, t] = hp
            act[l, :, t] = torch.stack(slots, 1)
        hn[l], cn[l] = hp, cp
    return hseq, act, hn, cn


def gate_grads(w: Sequence[Optional[Tensor]], h0: Optional[Tensor], c0: Optional[Tensor], hseq: Tensor, act: Tensor,
               dout: Optional[Tensor], dhn: Optional[Tensor], dcn: Optional[Tensor], H: int, NL: int, cell: int = 0,
               dtype=torch.float64):
    """BPTT on saved hseq / act: dg [NL, B, T, 4H] (pre-activation gate
    gradients), d(input of layer 0) [B, T, H-or-I columns of W_ih], dh0, dc0.
    dout [B, T, H] is the gradient of the top layer's output."""
    hseq, act = hseq.to(dtype), act.to(dtype)
    h0, c0, dout, dhn, dcn = (_cast(t, dtype) for t in (h0, c0, dout, dhn, dcn))
    _, B, T, _ = hseq.shape
    zero = hseq.new_zeros(B, H)
    dg = hseq.new_zeros(NL, B, T, 4 * H)
    dh0, dc0 = hseq.new_zeros(NL, B, H), hseq.new_zeros(NL, B, H)
    din = dout  # gradient arriving from above, [B, T, H] or None
    for l in range(NL - 1, -1, -1):
        w_ih, w_hh, _ = _layer(w, l, dtype)
        rec = dhn[l] if dhn is not None else zero           # W_hh^T dg of the step after
        carry = dcn[l] if (cell == 0 and dcn is not None) else zero  # LSTM: dc f; GRU: dh z
        for t in range(T - 1, -1, -1):
            a = act[l, :, t]
            dh = rec if din is None else rec + din[:, t]
            if cell == 0:
                i, f, g, o, c = a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]
                cp = act[l, :, t - 1, 4] if t > 0 else (c0[l] if c0 is not None else zero)
                tc = torch.tanh(c)
                dc = dh * o * (1 - tc * tc) + carry
                g4 = (dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o))
                carry = dc * f
            else:
                r, zg, nh, n = a[:, 0], a[:, 1], a[:, 3], a[:, 4]
                hp = hseq[l, :, t - 1] if t > 0 else (h0[l] if h0 is not None else zero)
                dh = dh + carry
                dpn = dh * (1 - zg) * (1 - n * n)
                g4 = (dpn * nh * r * (1 - r), dh * (hp - n) * zg * (1 - zg), dpn, dpn * r)
                carry = dh * zg
            dg[l, :, t] = torch.cat(g4, -1)
            rec = dg[l, :, t] @ w_hh
        dh0[l] = rec + carry if cell == 1 else rec
        if cell == 0:
            dc0[l] = carry
        din = dg[l] @ w_ih
    return dg, din, dh0, dc0


def layer_operands(x: Tensor, h0: Optional[Tensor], hseq: Tensor, l: int) -> Tuple[Tensor, Tensor]:
    """([B, T, I_l] input, [B, T, H] previous hidden state) of layer l."""
    B, T, H = hseq.shape[1:]
    first = (h0[l] if h0 is not None else hseq.new_zeros(B, H))[:, None]
    return (x if l == 0 else hseq[l - 1]), torch.cat([first, hseq[l, :, :-1]], 1)


def param_grads(dg: Tensor, x: Tensor, h0: Optional[Tensor], hseq: Tensor, has_bias: bool,
                rows: Optional[slice] = None) -> Tuple[Tensor, Tensor]:
    """(dparams, budget), flat in stack_layout's order.  rows: the batch rows
    that contribute (all)."""
    NL, B, T, _ = dg.shape
    n = B * T
    rows = rows if rows is not None else slice(None)
    grads: List[Tensor] = []
    budget: List[Tensor] = []
    for l in range(NL):
        g = dg[l, rows].reshape(-1, dg.shape[-1])
        ga = g.abs()
        ops = layer_operands(x, h0, hseq, l)
        for op in ops:
            o = op[rows].reshape(g.shape[0], -1)
            oa = o.abs()
            grads.append((g.t() @ o).reshape(-1))
            budget.append((ATOL * oa.sum(0)[None, :] + (RTOL + n * 2.0 ** -23) * (ga.t() @ oa)).reshape(-1))
        if has_bias:
            for _ in range(2):
                grads.append(g.sum(0))
                budget.append(ATOL * g.shape[0] + (RTOL + n * 2.0 ** -23) * ga.sum(0))
    return torch.cat(grads), torch.cat(budget)


def backward(x: Tensor, w: Sequence[Optional[Tensor]], h0: Optional[Tensor], c0: Optional[Tensor], hseq: Tensor,
             act: Tensor, dout: Optional[Tensor], dhn: Optional[Tensor], dcn: Optional[Tensor], H: int, NL: int,
             cell: int = 0, dtype=torch.float64):
    """dparams, budget, dx [B, T, I], dh0, dc0 (the GRU has no dc0: zeros)."""
    x, h0d, hs = x.to(dtype), _cast(h0, dtype), hseq.to(dtype)
    dg, dx, dh0, dc0 = gate_grads(w, h0, c0, hseq, act, dout, dhn, dcn, H, NL, cell, dtype)
    dparams, budget = param_grads(dg, x, h0d, hs, w[2] is not None)
    return dparams, budget, dx, dh0, dc0


def flat_offsets(w: Sequence[Optional[Tensor]], NL: int) -> List[Tuple[int, int, int, int]]:
    """Per layer the offsets of (dw_ih, dw_hh, db_ih, db_hh) in dparams (-1: no bias), then P."""
    out, off = [], 0
    for l in range(NL):
        row = []
        for k in range(4):
            t = w[4 * l + k]
            row.append(off if t is not None else -1)
            off += t.numel() if t is not None else 0
        out.append(tuple(row))
    return out + [(off,) * 4]
