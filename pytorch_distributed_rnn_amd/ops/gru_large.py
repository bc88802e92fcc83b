"""Large-hidden GRU stack on the MFMA step kernels (csrc/kernels/lstm_large.hip,
CELL = GRU).

New capability: the reference only builds ``nn.LSTM`` (reference:
src/motion/model.py:9), BASELINE.json names an "LSTM/GRU cell", and the
small-H GRU already runs on the fused kernels (ops/gru_fused.py).  This is the
16-bit, H % 64 == 0 counterpart for the shapes the large-H LSTM serves.

The GRU's gates ride on the LSTM step kernels' four-column quad as
``[r | z | n_x | n_h]`` (the layout of ops/gru_fused.py)::

    W_ih4 = [W_ir; W_iz; W_in; 0]      b4 = [b_ir + b_hr; b_iz + b_hz; b_in; b_hn]
    W_hh4 = [W_hr; W_hz; 0;    W_hn]

* forward: one library GEMM projects the input of all timesteps and both
  directions (``Xp = X W_ih4^T + b4``, gate-interleaved columns), then T
  launches of the MFMA step kernel whose epilogue applies
  ``r, z = sigma(.)``, ``n = tanh(n_x + r n_h)``, ``h = n + z (h_prev - n)``
  with ``h_prev`` kept in fp32;
* backward: T launches of the MFMA BPTT step (``dh_{t-1} = dgates_t W_hh4 +
  dh_t z_t``) emitting ``dgates = [dr r(1-r) | dz z(1-z) | dpre_n | dpre_n r]``
  in gate-blocked order, then ``dW_hh``, ``dW_ih``, the biases and ``dX`` as
  library GEMMs over all timesteps.

The zero blocks cost a quarter of the recurrent MFMA work; in exchange the GRU
shares every tile configuration, the split-K backward and the numerics tests
of the LSTM path.  Parameters stay in ``nn.GRU``'s layout (r, z, n).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import shadow as _sh
from .gemm import col_sum, mm_kk, mm_nk16
from .lstm_large import Cell, _state_grads, large_forward, supported  # noqa: F401  (supported: the same shapes)


def _hprev(hseq_d: Tensor, h0d: Optional[Tensor], d: int) -> Tensor:
    """h_{t-1} in processing order for direction d ([T, B, H])."""
    T, B, H = hseq_d.shape
    h0d = h0d if h0d is not None else hseq_d.new_zeros(1, B, H)
    return torch.cat([h0d, hseq_d[:-1]], 0) if d == 0 else torch.cat([hseq_d[1:], h0d], 0)


def _gru_shadows(weights, ndir: int, H: int, I: int, cdt, device):
    """The packed compute-dtype copies the kernels read -- per direction W_ih
    (dX GEMM), the [r | z | n_x | 0] projection stack (gate-interleaved, both
    directions concatenated), the [r | z | 0 | n_h] recurrent stack, its
    gate-interleaved form (forward step) and its transpose (BPTT step) -- plus
    the folded projection bias.  Cached on the first weight and rebuilt only
    when a parameter's version counter or storage changes (an optimizer step),
    like the large LSTM's shadows (ops/lstm_large.py:_shadow_cat)."""
    masters = list(weights[:4 * ndir])
    box = []

    def alloc():
        # buffers allocated once: the zero blocks stay zero, a rebuild after an
        # optimizer step only converts the parameters into them
        z = dict(device=device, dtype=cdt)
        box.append(([torch.empty(3 * H, I, **z) for _ in range(ndir)], torch.zeros(ndir * 4 * H, I, **z),
                    [torch.zeros(4 * H, H, **z) for _ in range(ndir)], [torch.zeros(4 * H, H, **z) for _ in range(ndir)],
                    [torch.zeros(H, 4 * H, **z) for _ in range(ndir)],
                    torch.zeros(ndir * 4 * H, device=device, dtype=torch.float32)))
        return box[0]

    def build(*ms):
        # every job reads a master, never another output of the same launch
        wih, wih4_all, whh4, whh_p, wt, b4_all = box[0]
        jobs = []
        for d in range(ndir):
            w_ih, w_hh, b_ih, b_hh = ms[4 * d:4 * d + 4]
            wh = w_hh.view(3, H, H)
            jobs.append(_sh.job(wih[d], w_ih))
            # projection stack [r | z | n_x | 0], gate-interleaved: row 4u + q
            jobs.append(_sh.job(wih4_all[d * 4 * H:(d + 1) * 4 * H].view(H, 4, I)[:, :3],
                                w_ih.view(3, H, I).transpose(0, 1)))
            # recurrent stack [r | z | 0 | n_h] (gate-blocked), its interleaved
            # form and its transpose
            jobs.append(_sh.job(whh4[d][:2 * H], w_hh[:2 * H]))
            jobs.append(_sh.job(whh4[d][3 * H:], w_hh[2 * H:]))
            jobs.append(_sh.job(whh_p[d].view(H, 4, H)[:, :2], wh[:2].transpose(0, 1)))
            jobs.append(_sh.job(whh_p[d].view(H, 4, H)[:, 3], wh[2]))
            jobs.append(_sh.job(wt[d][:, :2 * H], w_hh[:2 * H].t()))
            jobs.append(_sh.job(wt[d][:, 3 * H:], w_hh[2 * H:].t()))
            # folded bias [b_ir + b_hr | b_iz + b_hz | b_in | b_hn], interleaved
            b = b4_all[d * 4 * H:(d + 1) * 4 * H].view(H, 4)
            bi = b_ih.view(3, H).t() if b_ih is not None else None
            bh = b_hh.view(3, H).t() if b_hh is not None else None
            if bi is not None and bh is not None:
                jobs.append(_sh.job(b[:, :2], bi[:, :2], bh[:, :2]))
            elif bi is not None or bh is not None:
                jobs.append(_sh.job(b[:, :2], (bi if bi is not None else bh)[:, :2]))
            if bi is not None:
                jobs.append(_sh.job(b[:, 2], bi[:, 2]))
            if bh is not None:
                jobs.append(_sh.job(b[:, 3], bh[:, 2]))
        return jobs

    return _sh.get(weights[0], ("gru", cdt, ndir, H, I), masters, alloc, build)


def _shadows(weights, ndir: int, H: int, I: int, cdt, device):
    wih, wih4_all, _, whh_p, wt, b4_all = _gru_shadows(weights, ndir, H, I, cdt, device)
    return wih4_all, b4_all, whh_p, wih, wt


def _db_hh(rs: Tensor, G: Tensor, H: int, out: Tensor) -> Tensor:
    """b_hh's gradient out of the row sums of the dW_ih pass (over [r | z |
    dpre_n]) and dgates G: [rs[:2H] | column sums of the n_h block]."""
    out[:2 * H].copy_(rs[:2 * H])
    out[2 * H:].copy_(col_sum(G[:, 3 * H:]))
    return out


def _backward_gemms16(ctx, dgates, dh0, dc0, hseq, h0c, x2, wih):
    """16-bit layers: weight and input gradients on the in-tree MFMA GEMM
    (ops/gemm.py), dW_hh against a concatenated h_prev and over all four
    column blocks, its n_x block dropped afterwards.  The LSTM's counterpart
    (ops/lstm_large.py:_backward_gemms16) pairs shifted views as K segments
    and can accumulate into the flat gradients (gradsink) instead; converging
    the two changes this path's launches and speed, so it is a change of its
    own."""
    cell, H, ndir, tile, rev_mask, has_w, h0_dtype, _ = ctx.cfg
    T, B = hseq.shape[:2]
    grads: List[Optional[Tensor]] = []
    dx_pairs = []
    for d in range(ndir):
        G = dgates[d].view(T * B, 4 * H)                         # [r | z | dpre_n | dpre_n r]
        Gx = G[:, :3 * H]                                        # x side: [r | z | dpre_n]
        hprev = _hprev(hseq[:, :, d * H:(d + 1) * H], h0c[d:d + 1] if h0c is not None else None, d)
        dw4 = mm_kk([(G, hprev.reshape(T * B, H))])
        dwih = mm_kk([(Gx, x2)])
        cs = col_sum(G)
        dbih = cs[:3 * H]
        dwhh, dbhh = dw4.new_empty(3 * H, H), cs.new_empty(3 * H)  # nn.GRU has no n_x block in W_hh
        for dst, src in ((dwhh, dw4), (dbhh, cs)):
            dst[:2 * H].copy_(src[:2 * H])
            dst[2 * H:].copy_(src[3 * H:])
        dx_pairs.append((Gx, wih[d]))
        grads += [dwih, dwhh, dbih if has_w[4 * d + 2] else None, dbhh if has_w[4 * d + 3] else None]
    # both directions' dX in one launch
    dx = mm_nk16(dx_pairs).view(T, B, x2.shape[1]) if ctx.needs_input_grad[0] else None
    return (dx, *_state_grads(ctx, dh0, None, h0_dtype, None), None, *grads)


# gates r, z, n on the quad [r | z | n_x | n_h]: the x side is its first three
# blocks, and nn.GRU's W_hh [r | z | n] takes the [r | z] and n_h blocks
GRU = Cell(cell=1, gates=3, has_c=False, xcols=3, hh_blocks=((0, 2, 0), (3, 4, 2)), db_hh=_db_hh, shadows=_shadows,
           backward16=_backward_gemms16)


def gru_large_forward(x: Tensor, weights: Sequence[Optional[Tensor]], h0: Optional[Tensor],
                      **kw) -> Tuple[Tensor, Tensor]:
    """Stacked (bi)GRU on the MFMA step kernels; ``nn.GRU``-compatible outputs
    (ops/lstm_large.py:large_forward's keywords)."""
    out, hn, _ = large_forward(GRU, x, weights, h0, None, **kw)
    return out, hn

