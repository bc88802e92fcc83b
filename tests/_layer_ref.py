"""fp64 reference of the host contract of one large-H layer: what
ops/lstm_large.py (_LargeLayer, _PipelinedStack, _weight_grads,
_backward_gemms16) and ops/gru_large.py make of the recurrence bindings'
operands and results.  Plain torch, no extension import:
tests/test_layer_ref_cpu.py proves this file against fp64 autograd of
torch.nn.LSTM / torch.nn.GRU, tests/test_gpu_large_layer_exact.py checks the
host code against this file.

It works from the tensors the recurrence received and returned (the layer
input x, h0, and the kernel's own hseq / dgates), so no rounding of the
recurrence enters a comparison -- the teacher forcing of _large_ref.py, one
tier up.  Everything is in nn.LSTM / nn.GRU layout: per direction d
(direction 1 runs reversed) W_ih [gates*H, I], W_hh [gates*H, H], b_ih, b_hh
[gates*H]; dgates [ndir, T, B, 4H] gate-blocked, for the GRU on the quad
[r | z | n_x | n_h].

A :class:`Product` carries, beside the exact value, the ``|A| |B|`` matrix
and the number of terms of its sum: the operands of the forward error bound

    |got - ref| <= (terms + S + 1) 2^-23 (|A| |B|)  (+ u16 |ref|, 16-bit result)

of tests/_gemm_ref.py:bound_ratio (S: K splits), see :func:`ratio`.  A term
that is not a product (the folded bias, the old value of an accumulated
gradient) counts as one more term of magnitude |term|.  The folded bias is
itself an fp32 sum b_ih + b_hh: its rounding, 2^-24 (|b_ih| + |b_hh|), is
inside one term of 2^-23 (|b_ih| + |b_hh|), so the bias enters ``absprod`` as
|b_ih| + |b_hh|.
"""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

import _large_ref as L

U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# cell id of the bindings -> (gate rows of the parameters, x-side blocks of dgates,
# dgates row blocks [b0, b1) that make up dW_hh / db_hh, in units of H)
CELLS = {0: (4, 4, ((0, 4),)), 1: (3, 3, ((0, 2), (3, 4)))}

Params = Tuple[Tensor, Tensor, Optional[Tensor], Optional[Tensor]]  # w_ih, w_hh, b_ih, b_hh of one direction


class Product(NamedTuple):
    ref: Tensor      # exact value, fp64
    absprod: Tensor  # |A| |B| (+ |extra terms|), fp64
    terms: int       # terms of the sum


def product(A: Tensor, B: Tensor) -> Product:
    """A [M, K] B[N, K]^T."""
    A, B = A.double(), B.double()
    return Product(A @ B.t(), A.abs() @ B.abs().t(), A.shape[1])


def plus(p: Product, term: Tensor, mag: Optional[Tensor] = None) -> Product:
    """One more term (broadcast) of magnitude ``mag`` (default |term|)."""
    term = term.double()
    return Product(p.ref + term, p.absprod + (term.abs() if mag is None else mag.double()), p.terms + 1)


def _rows(p: Product, H: int, blocks) -> Product:
    """Row blocks [b0*H, b1*H) of a product, concatenated."""
    pick = lambda t: torch.cat([t[b0 * H:b1 * H] for b0, b1 in blocks], 0)
    return Product(pick(p.ref), pick(p.absprod), p.terms)


def ratio(got: Tensor, p: Product, S: int, extra: Optional[Tensor] = None) -> float:
    """max |got - ref| / bound, bound = (terms + S + 1) 2^-23 absprod, + u16
    |ref| for a 16-bit result, + ``extra`` (a named further rounding).  An
    element whose bound is zero must be exact (ratio 0, else inf)."""
    g = got.detach().cpu()
    assert g.shape == p.ref.shape, (g.shape, p.ref.shape)
    assert not torch.isnan(g).any(), "NaN"
    if g.numel() == 0:
        return 0.0
    bound = (p.terms + S + 1) * 2.0 ** -23 * p.absprod
    if g.dtype != torch.float32:
        bound = bound + U16[g.dtype] * p.ref.abs()
    if extra is not None:
        bound = bound + extra
    err = (g.double() - p.ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item()


# ---------------------------------------------------------------- packed operands
class Packed(NamedTuple):
    proj: Tensor          # [ndir*4H, I] gate-interleaved W_ih of every direction (the GRU's n_h rows zero)
    bias: Tensor          # [ndir*4H] fp64 folded bias, interleaved
    bias_mag: Tensor      # its magnitude for the bound (|b_ih| + |b_hh| where two are folded)
    w: List[Tensor]       # per direction [4H, H] interleaved W_hh (lstm_large_fwd / lstm_rows_fwd_range)
    wt: List[Tensor]      # per direction [H, 4H] W_hh^T, gate-blocked columns (the BPTT bindings)
    wih: List[Tensor]     # per direction W_ih as stored (the dX product)


def packed(cell: int, params: Sequence[Params], H: int) -> Packed:
    """The operands of one layer from its parameters, weights already rounded
    to the compute dtype (kept in that dtype: the packing only permutes and
    inserts zeros), biases as the fp32 masters."""
    pack = L.lstm_pack if cell == 0 else L.gru_pack
    proj, bias, mag, w, wt, wih = [], [], [], [], [], []
    for w_ih, w_hh, b_ih, b_hh in params:
        pi, pw, pwt, _ = pack(w_ih, w_hh, None, None, H)
        d64 = lambda t: None if t is None else t.detach().double()
        a64 = lambda t: None if t is None else t.detach().double().abs()
        proj.append(pi)
        w.append(pw.contiguous())
        wt.append(pwt)
        wih.append(w_ih)
        bias.append(pack(w_ih.double(), w_hh.double(), d64(b_ih), d64(b_hh), H)[3])
        mag.append(pack(w_ih.double(), w_hh.double(), a64(b_ih), a64(b_hh), H)[3])
    return Packed(torch.cat(proj, 0), torch.cat(bias), torch.cat(mag), w, wt, wih)


def xp(x: Tensor, pk: Packed) -> Product:
    """[T*B, ndir*4H]: x W_ih_packed^T + b_packed, every direction."""
    x2 = x.reshape(-1, x.shape[-1])
    return plus(product(x2, pk.proj), pk.bias, pk.bias_mag)


# ---------------------------------------------------------------- gradients
class LayerGrads(NamedTuple):
    params: List[Dict[str, Product]]  # per direction: dW_ih, dW_hh, db_ih, db_hh
    dx: Product                       # [T*B, I], every direction summed
    dx_parts: List[Product]           # one direction's share each


def grads(cell: int, dgates: Tensor, hseq: Tensor, h0: Optional[Tensor], x: Tensor, wih: Sequence[Tensor],
          H: int) -> LayerGrads:
    """dgates [ndir, T, B, 4H], hseq [T, B, ndir*H], h0 [ndir, B, H] or None,
    x [T, B, I], wih: per direction W_ih as stored (compute dtype)."""
    _, xcols, hh_blocks = CELLS[cell]
    ndir, T, B, _ = dgates.shape
    x2 = x.double().reshape(T * B, -1)
    ones = x2.new_ones(1, T * B)
    hseq = hseq.double()
    h0 = h0.double() if h0 is not None else None
    out, Gxs = [], []
    for d in range(ndir):
        rev = d == 1
        G = dgates[d].double().reshape(T * B, 4 * H)
        hp = L.h_prev(hseq, h0, d, H, rev).reshape(T * B, H)
        keep = slice(0, T * B)
        if h0 is None:  # the step next to the absent state has no term in dW_hh
            keep = slice(0, (T - 1) * B) if rev else slice(B, T * B)
        dw4 = product(G[keep].t(), hp[keep].t())     # einsum("tbg,tbh->gh", dgates_d, h_prev)
        Gx = G[:, :xcols * H]
        cs = product(G.t(), ones)
        cs = Product(cs.ref[:, 0], cs.absprod[:, 0], cs.terms)
        out.append({"dW_ih": product(Gx.t(), x2.t()), "dW_hh": _rows(dw4, H, hh_blocks),
                    "db_ih": _rows(cs, H, ((0, xcols),)), "db_hh": _rows(cs, H, hh_blocks)})
        Gxs.append(Gx)
    parts = [product(Gxs[d], wih[d].double().t()) for d in range(ndir)]
    dx = product(torch.cat(Gxs, 1), torch.cat([w.double().t() for w in wih], 1))
    return LayerGrads(out, dx, parts)
