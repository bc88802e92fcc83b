"""tests/_layer_ref.py (the fp64 reference of the large-H layer host code)
against fp64 autograd of torch.nn.LSTM / torch.nn.GRU, on the CPU.

Fed the free-running fp64 results of tests/_large_ref.py (nothing rounded),
its packed input projection drives the recurrence to torch's outputs, and its
weight, bias and input gradients equal torch's to 1e-10, the tolerance of
test_reference_matches_torch_fp64."""
import pytest
import torch

import _gemm_ref as GR
import _large_ref as L
import _layer_ref as LR

F64 = torch.float64
TOL = dict(rtol=0, atol=1e-10)


def _params(m, d, bias):
    sfx = "_l0" + ("_reverse" if d else "")
    return (getattr(m, "weight_ih" + sfx), getattr(m, "weight_hh" + sfx),
            getattr(m, "bias_ih" + sfx) if bias else None, getattr(m, "bias_hh" + sfx) if bias else None)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("cell", [0, 1])
def test_layer_reference_matches_torch_fp64(cell, ndir, bias, state, T):
    torch.manual_seed(100 * cell + 10 * ndir + 2 * bias + state + T)
    H, B, I = 5, 3, 6
    lstm = cell == 0
    m = (torch.nn.LSTM if lstm else torch.nn.GRU)(I, H, 1, bias=bias, bidirectional=ndir == 2).double()
    x = torch.randn(T, B, I, dtype=F64, requires_grad=True)
    h0 = torch.randn(ndir, B, H, dtype=F64, requires_grad=True) if state else None
    c0 = torch.randn(ndir, B, H, dtype=F64, requires_grad=True) if state and lstm else None
    if lstm:
        out, (hn, cn) = m(x, (h0, c0) if state else None)
    else:
        out, hn = m(x, h0)
        cn = None
    g, ghn = torch.randn_like(out), torch.randn_like(hn)
    gcn = torch.randn_like(cn) if lstm else None
    torch.autograd.backward([out, hn] + ([cn] if lstm else []), [g, ghn] + ([gcn] if lstm else []))

    mask = 2 if ndir == 2 else 0
    with torch.no_grad():
        params = [tuple(p.detach() if p is not None else None for p in _params(m, d, bias)) for d in range(ndir)]
        pk = LR.packed(cell, params, H)
        for d in range(ndir):  # the two layouts of one matrix; the GRU's zero blocks
            assert torch.equal(L.wt_of(pk.w[d], H), pk.wt[d])
            if not lstm:
                assert not pk.wt[d][:, 2 * H:3 * H].any() and not pk.proj[d * 4 * H:(d + 1) * 4 * H].view(H, 4, I)[:, 3].any()
        xp = LR.xp(x.detach(), pk)
        assert xp.terms == I + 1
        h0d = h0.detach() if state else None
        s0d = (c0 if lstm else h0).detach() if state else None
        hseq, cseq, acts = L.forward(xp.ref.view(T, B, ndir * 4 * H), pk.w, h0d, s0d, H, mask, cell)
        torch.testing.assert_close(hseq, out.detach(), **TOL)
        dgates, dh0, dc0 = L.backward(g, ghn, gcn, pk.wt, cseq, acts, s0d, H, mask, cell)
        lg = LR.grads(cell, dgates, hseq, h0d, x.detach(), pk.wih, H)
        torch.testing.assert_close(lg.dx.ref.view(T, B, I), x.grad, **TOL)
        torch.testing.assert_close(sum(p.ref for p in lg.dx_parts), lg.dx.ref, **TOL)
        for d in range(ndir):
            w_ih, w_hh, b_ih, b_hh = _params(m, d, bias)
            got = lg.params[d]
            torch.testing.assert_close(got["dW_ih"].ref, w_ih.grad, **TOL)
            torch.testing.assert_close(got["dW_hh"].ref, w_hh.grad, **TOL)
            assert got["dW_ih"].terms == T * B and got["dW_hh"].terms == (T if state else T - 1) * B
            if bias:
                torch.testing.assert_close(got["db_ih"].ref, b_ih.grad, **TOL)
                torch.testing.assert_close(got["db_hh"].ref, b_hh.grad, **TOL)
            for p in got.values():  # |A| |B| dominates the value it bounds
                assert (p.absprod >= p.ref.abs() - 1e-12).all()
        if not state and T == 1:
            assert all(not lg.params[d]["dW_hh"].ref.any() and not lg.params[d]["dW_hh"].absprod.any() for d in range(ndir))
        if state:
            torch.testing.assert_close(dh0, h0.grad, **TOL)


def test_ratio_is_the_gemm_bound():
    """ratio() on a plain product is _gemm_ref.bound_ratio; a further term
    widens it by that term alone; a zero bound demands an exact result."""
    g = GR.gen(3)
    A, B = torch.randn(7, 33, generator=g, dtype=F64), torch.randn(5, 33, generator=g, dtype=F64)
    p = LR.product(A, B)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        got = (p.ref * (1 + 2.0 ** -12)).to(dtype)
        assert LR.ratio(got, p, 3) == pytest.approx(GR.bound_ratio(got, A, B, 3), rel=1e-12)
    b = torch.randn(5, generator=g, dtype=F64)
    q = LR.plus(p, b)
    assert q.terms == 34 and torch.equal(q.ref, p.ref + b) and torch.equal(q.absprod, p.absprod + b.abs())
    z = LR.product(torch.zeros(4, 0), torch.zeros(3, 0))
    assert LR.ratio(torch.zeros(4, 3), z, 1) == 0.0
    assert LR.ratio(torch.full((4, 3), 1e-30), z, 1) == float("inf")
