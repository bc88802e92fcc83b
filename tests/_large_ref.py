"""fp64 reference of the large-H recurrence contract (lstm_large_fwd /
lstm_large_bwd in csrc/bindings.cpp, as ops/lstm_large.py and ops/gru_large.py
call them).  Plain torch, no extension import: tests/test_gpu_lstm_large_steps.py
checks this file against fp64 torch.nn.LSTM / torch.nn.GRU on the CPU and the
kernels against this file on the GPU.

Layouts (H hidden units, 4 gate slots q per unit u):
  xp    [T, B, ndir*4H]  input projection, bias included, per direction
                         gate-interleaved (column 4u + q)
  w[d]  [4H, H]          recurrent weight, gate-interleaved rows
  wt[d] [H, 4H]          its transpose with gate-BLOCKED columns (q*H + u)
  h0    [ndir, B, H]     state entering the step GEMM;  c0 [ndir, B, H] state
                         entering the cell (LSTM: c; GRU: the fp32 copy of h)
  hseq  [T, B, ndir*H]   cseq [ndir, T, B, H]   acts [ndir, T, B, 4H] interleaved
  dgates [ndir, T, B, 4H] gate-blocked;  dh0, dc0 [ndir, B, H]
  reverse_mask: bit d set = direction d runs from T-1 down to 0.
cell 0 = LSTM, slots (i, f, g, o).  cell 1 = GRU, slots (r, z, n_x, n_h) with
  n = tanh(n_x + r n_h),  h = n + z (h_prev - n);
acts keeps (r, z, n, n_h): n in n_x's slot, n_h linear.

Every function runs step by step in the dtype of its arguments' ``.double()``
copies.  ``forced`` arguments switch a step's recurrent input from the
reference's own previous result to a given tensor (teacher forcing): with the
kernel's stored outputs there, each step is compared on identical inputs and
no rounding of an earlier step leaks into a later one.  The carries no kernel
returns (LSTM dc f, GRU dh z) always run free, in fp64, across all steps.
"""
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor


def interleave_rows(w: Tensor, H: int) -> Tensor:
    """dst[4u + q] = src[q*H + u] (ops/lstm_large.py _interleave_job)."""
    return w.reshape(4, H, -1).transpose(0, 1).reshape(w.shape)


def deinterleave_rows(w: Tensor, H: int) -> Tensor:
    """dst[q*H + u] = src[4u + q]."""
    return w.reshape(H, 4, -1).transpose(0, 1).reshape(w.shape)


def wt_of(w: Tensor, H: int) -> Tensor:
    """The backward's operand for a gate-interleaved recurrent weight."""
    return deinterleave_rows(w, H).t().contiguous()


def lstm_pack(w_ih: Tensor, w_hh: Tensor, b_ih: Optional[Tensor], b_hh: Optional[Tensor], H: int):
    """nn.LSTM parameters of one direction -> (W_ih interleaved, w, wt, bias interleaved)."""
    b = w_ih.new_zeros(4 * H)
    for t in (b_ih, b_hh):
        if t is not None:
            b = b + t
    return interleave_rows(w_ih, H), interleave_rows(w_hh, H), w_hh.t().contiguous(), interleave_rows(b, H)


def gru_pack(w_ih: Tensor, w_hh: Tensor, b_ih: Optional[Tensor], b_hh: Optional[Tensor], H: int):
    """nn.GRU parameters (r, z, n) on the quad (ops/gru_large.py):
    W_ih4 = [W_ir; W_iz; W_in; 0], W_hh4 = [W_hr; W_hz; 0; W_hn],
    b4 = [b_ir + b_hr; b_iz + b_hz; b_in; b_hn]."""
    zi, zh = w_ih.new_zeros(H, w_ih.shape[1]), w_hh.new_zeros(H, H)
    bi = b_ih if b_ih is not None else w_ih.new_zeros(3 * H)
    bh = b_hh if b_hh is not None else w_ih.new_zeros(3 * H)
    w_ih4 = torch.cat([w_ih, zi], 0)
    w_hh4 = torch.cat([w_hh[:2 * H], zh, w_hh[2 * H:]], 0)
    b4 = torch.cat([bi[:2 * H] + bh[:2 * H], bi[2 * H:], bh[2 * H:]], 0)
    return interleave_rows(w_ih4, H), interleave_rows(w_hh4, H), w_hh4.t().contiguous(), interleave_rows(b4, H)


def _order(T: int, rev: bool) -> List[int]:
    return list(range(T - 1, -1, -1)) if rev else list(range(T))


def _f64(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.double()


def forward(xp: Tensor, w: Sequence[Tensor], h0: Optional[Tensor], c0: Optional[Tensor], H: int, reverse_mask: int,
            cell: int, forced: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """hseq, cseq, acts in fp64.  forced = (hseq, cseq): a step's incoming state
    is taken from these tensors (the step before it in processing order)."""
    T, B, _ = xp.shape
    ndir = len(w)
    xp, h0, c0 = xp.double(), _f64(h0), _f64(c0)
    hseq = xp.new_zeros(T, B, ndir * H)
    cseq = xp.new_zeros(ndir, T, B, H)
    acts = xp.new_zeros(ndir, T, B, 4 * H)
    src_h, src_c = (forced[0].double(), forced[1].double()) if forced is not None else (hseq, cseq)
    zero = xp.new_zeros(B, H)
    for d in range(ndir):
        wd = w[d].double()
        prev = None
        for t in _order(T, bool(reverse_mask & (1 << d))):
            if prev is None:
                hp = h0[d] if h0 is not None else zero
                cp = c0[d] if c0 is not None else zero
            else:
                hp, cp = src_h[prev, :, d * H:(d + 1) * H], src_c[d, prev]
            z = (xp[t, :, d * 4 * H:(d + 1) * 4 * H] + hp @ wd.t()).view(B, H, 4)
            if cell == 0:
                i, f, o = torch.sigmoid(z[..., 0]), torch.sigmoid(z[..., 1]), torch.sigmoid(z[..., 3])
                g = torch.tanh(z[..., 2])
                c = f * cp + i * g
                h = o * torch.tanh(c)
                quad = (i, f, g, o)
            else:
                r, zg, nh = torch.sigmoid(z[..., 0]), torch.sigmoid(z[..., 1]), z[..., 3]
                n = torch.tanh(z[..., 2] + r * nh)
                c = h = n + zg * (cp - n)
                quad = (r, zg, n, nh)
            hseq[t, :, d * H:(d + 1) * H] = h
            cseq[d, t] = c
            acts[d, t] = torch.stack(quad, -1).view(B, 4 * H)
            prev = t
    return hseq, cseq, acts


def backward(dout: Optional[Tensor], dhn: Optional[Tensor], dcn: Optional[Tensor], wt: Sequence[Tensor], cseq: Tensor,
             acts: Tensor, c0: Optional[Tensor], H: int, reverse_mask: int, cell: int,
             forced: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """dgates, dh0, dc0 in fp64 from the saved cseq / acts (cell_bwd_elem's
    formulas).  forced = dgates: the recurrent dh of a step is that tensor's
    entry of the step processed before it, times W.  The GRU has no dc0 (zeros)."""
    ndir, T, B, _ = acts.shape
    cseq, acts = cseq.double(), acts.double()
    dout, dhn, dcn, c0 = _f64(dout), _f64(dhn), _f64(dcn), _f64(c0)
    dgates = acts.new_zeros(ndir, T, B, 4 * H)
    dh0 = acts.new_zeros(ndir, B, H)
    dc0 = acts.new_zeros(ndir, B, H)
    src = forced.double() if forced is not None else dgates
    zero = acts.new_zeros(B, H)
    for d in range(ndir):
        W = wt[d].double().t()                                   # [4H, H], gate-blocked rows
        fwd_order = _order(T, bool(reverse_mask & (1 << d)))
        dh = dhn[d] if dhn is not None else zero                # recurrent part entering the step
        carry = dcn[d] if (cell == 0 and dcn is not None) else zero
        for k in range(T - 1, -1, -1):
            t = fwd_order[k]
            a = acts[d, t].view(B, H, 4)
            sp = cseq[d, fwd_order[k - 1]] if k > 0 else (c0[d] if c0 is not None else zero)
            if dout is not None:
                dh = dh + dout[t, :, d * H:(d + 1) * H]
            if cell == 0:
                ig, fg, gg, og = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
                tc = torch.tanh(cseq[d, t])
                dc = dh * og * (1 - tc * tc) + carry
                dg = (dc * gg * ig * (1 - ig), dc * sp * fg * (1 - fg), dc * ig * (1 - gg * gg), dh * tc * og * (1 - og))
                carry = dc * fg
            else:
                r, zg, n, nh = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
                dh = dh + carry
                dpn = dh * (1 - zg) * (1 - n * n)
                dg = (dpn * nh * r * (1 - r), dh * (sp - n) * zg * (1 - zg), dpn, dpn * r)
                carry = dh * zg
            dgates[d, t] = torch.cat(dg, -1)
            dh = src[d, t] @ W
        dh0[d] = dh + carry if cell == 1 else dh
        if cell == 0:
            dc0[d] = carry
    return dgates, dh0, dc0


def h_prev(hseq: Tensor, h0: Optional[Tensor], d: int, H: int, rev: bool) -> Tensor:
    """[T, B, H]: the state each step of direction d consumed."""
    hd = hseq[:, :, d * H:(d + 1) * H]
    first = (h0[d] if h0 is not None else torch.zeros_like(hd[0]))[None]
    return torch.cat([hd[1:], first], 0) if rev else torch.cat([first, hd[:-1]], 0)
