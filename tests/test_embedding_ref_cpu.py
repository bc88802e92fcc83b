"""The references of tests/_embedding_ref.py against independent formulas on
the CPU: fp64 ``F.embedding`` and its autograd (negative indices, padding),
``torch.sort(stable=True)``; and the exactness claim the GPU tests rest on:
fp32 sums of dyadic rows are bit-equal in any order and equal the fp64 sum."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _embedding_ref as E


@pytest.mark.parametrize("pad", [None, 2, -1])
def test_gather_and_scatter_add_match_fp64_autograd(pad):
    g = E.gen(1)
    V, D, T, B = 7, 5, 11, 3
    w = torch.randn(V, D, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(-V, V, (T, B), generator=g)
    idx[0, 0], idx[1, 1] = 2, V - 1      # both padding rows have contributions
    dout = torch.randn(T, B, D, generator=g, dtype=torch.float64)
    out = F.embedding(E.wrap(idx, V), w, padding_idx=pad)   # F.embedding itself takes no negative index
    out.backward(dout)
    assert torch.equal(E.gather(w.detach(), idx), out.detach())
    ref = E.scatter_add(dout, idx, V, pad)
    assert torch.allclose(ref, w.grad, rtol=0, atol=1e-13)
    if pad is not None:
        assert ref[pad].abs().max() == 0 and w.grad[pad].abs().max() == 0
    base = torch.randn(V, D, generator=g, dtype=torch.float64)
    withbase = E.scatter_add(dout, idx, V, pad, base)
    assert torch.equal(withbase, base + ref)
    if pad is not None:
        assert torch.equal(withbase[pad], base[pad])


@pytest.mark.parametrize("V,N", [(1, 300), (5, 257), (300, 4097), (7, 0), (16384, 5000)])
def test_stable_sort_matches_torch(V, N):
    g = E.gen(V + N)
    idx = torch.randint(-V, V, (N,), generator=g)
    perm, off = E.stable_sort(idx, V)
    vals, ref_perm = torch.sort(E.wrap(idx, V), stable=True)
    assert torch.equal(perm, ref_perm)
    assert torch.equal(off, torch.searchsorted(vals, torch.arange(V + 1)))
    assert off[0] == 0 and off[-1] == N


def test_dyadic_sums_are_exact_in_fp32_in_any_order():
    """n = 2**16 rows of m / 8, |m| <= 16: the fp32 running sum in four random
    orders, a pairwise sum and the fp64 sum all agree bit for bit.  (The
    argument covers n up to 2**19; 2**16 keeps this quick.)"""
    g = E.gen(3)
    n, D = 2 ** 16, 8
    rows = E.dyadic_rows((n, D), g)
    assert torch.equal(rows.float().double(), rows) and torch.equal(rows.bfloat16().double(), rows) \
        and torch.equal(rows.half().double(), rows)
    ref = rows.sum(0)
    assert ref.abs().max().item() <= 2 * n and torch.equal((ref * 8).round(), ref * 8)
    r32 = rows.float().numpy()
    for k in range(4):
        order = torch.randperm(n, generator=g).numpy()
        run = np.cumsum(r32[order], axis=0, dtype=np.float32)[-1]   # a sequential fp32 sum
        assert np.array_equal(run.astype(np.float64), ref.numpy()), k
    assert torch.equal(rows.float().sum(0).double(), ref)            # torch's blocked / pairwise order
    # the largest case the argument is used for: all terms at the magnitude limit
    assert 16 * E.N_MAX < 2 ** 24
    big = np.float32(2.0 * E.N_MAX - 2.0)
    assert np.float32(big + np.float32(2.0)) == np.float64(2.0 * E.N_MAX) and np.float32(big + np.float32(0.125)) - big == 0.125


def test_special_values_table_is_what_it_says():
    v = E.special_values()
    b = E.special_bits()
    assert torch.equal(E.bits(v).long() & 0xffffffff, b)
    fin = torch.isfinite(v)
    assert int(torch.isnan(v).sum()) == 6 and int(torch.isinf(v).sum()) == 2
    assert not ((v[fin] != 0) & (v[fin].abs() < 2.0 ** -126)).any(), "an fp32 subnormal in the table"
    f = lambda bits: v[(b == bits).nonzero()[0, 0]]
    assert f(0x477fe000).item() == 65504.0 and f(0x477ff000).item() == 65520.0
    assert f(0x477ff000).half().isinf() and f(0x477fefff).half().item() == 65504.0
    assert f(0x3f808000).bfloat16().item() == 1.0 and f(0x3f818000).bfloat16().item() == 1.015625
    assert f(0x3f801000).half().item() == 1.0 and f(0x3f803000).half().item() == 1.0 + 2.0 ** -9
    assert f(0x33000000).half().item() == 0.0 and f(0x33000001).half().item() == 2.0 ** -24
    assert f(0x33c00000).half().item() == 2.0 ** -23 and f(0x387fe000).half().item() == 2.0 ** -14
    assert f(0x7f7fffff).bfloat16().isinf() and f(0x7f7f8000).bfloat16().isinf() and f(0x7f7f0000).bfloat16().isfinite()


def test_assert_bits_sees_zero_signs_and_ignores_nan_payloads():
    a = torch.tensor([0.0, float("nan"), 1.0])
    E.assert_bits(a, a.clone())
    with pytest.raises(AssertionError):
        E.assert_bits(torch.tensor([-0.0, float("nan"), 1.0]), a)
    with pytest.raises(AssertionError):
        E.assert_bits(torch.tensor([0.0, 2.0, 1.0]), a)
