"""CPU: the exactness argument of tests/_gemm_ref.py rests on the operands,
not on a kernel: dyadic values are exact in every dtype, every prefix of an
fp32 sum of their products -- in several shuffled orders, at the longest K the
argument covers and at the largest magnitudes -- equals the fp64 sum, and the
integer mirrors of the kernels' index arithmetic have the properties the GPU
tests rely on."""
import pytest
import torch

import _gemm_ref as R


def test_value_set_exact_in_every_dtype():
    v = torch.arange(-R.MAG, R.MAG + 1).double() / R.SCALE
    g = R.dyadic(64, 64, R.gen(0))
    assert set(g.flatten().tolist()) <= set(v.tolist())
    assert g.min() == -2 and g.max() == 2          # both extremes drawn
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(v.to(dt).double(), v)
    prod = v[:, None] * v[None, :]
    assert torch.equal(prod * 64, (prod * 64).round()) and prod.abs().max() == 4
    # products of the 16-bit values are exact in fp32 as well
    assert torch.equal((v.float()[:, None] * v.float()[None, :]).double(), prod)


@pytest.mark.parametrize("worst", [False, True])
def test_fp32_sums_exact_in_any_order(worst):
    K = R.K_MAX
    g = R.gen(1)
    if worst:   # every product +4 (or -4): the largest partial sums the bound allows
        a = torch.full((K,), 2.0, dtype=torch.float64)
        b = a.clone()
    else:
        a, b = R.dyadic(1, K, g)[0], R.dyadic(1, K, g)[0]
    p64 = a * b
    p32 = a.float() * b.float()
    assert torch.equal(p32.double(), p64)
    total = p64.sum()
    for trial in range(6):
        perm = torch.randperm(K, generator=g)
        pre32 = torch.cumsum(p32[perm], 0, dtype=torch.float32)     # every partial sum of this order
        pre64 = torch.cumsum(p64[perm], 0)
        assert torch.equal(pre32.double(), pre64), trial
        # a sequential loop in fp32 (no library reduction order involved)
        s = torch.zeros((), dtype=torch.float32)
        for x in p32[perm][:2048]:
            s = s + x
        assert s.double() == pre64[2047]
        # tree orders: sums of 8 / 64 / 512 blocks, then of the block sums
        for blk in (8, 64, 512):
            part = p32[perm].view(-1, blk).sum(1, dtype=torch.float32)
            assert torch.equal(part.double(), p64[perm].view(-1, blk).sum(1))
            assert part.sum(dtype=torch.float32).double() == total
    # with an integer bias and a dyadic accumulate base on top
    assert (torch.tensor(4.0 * K + 1000 + 2).float().double() == 4.0 * K + 1002)
    assert 4.0 * K + 1002 < 2 ** 24 * 2 ** -6


def test_round16_is_one_round_to_nearest_even():
    ties = torch.tensor([257.0, 259.0, -257.0, 2049.0, 2051.0, 2050.0], dtype=torch.float64)
    assert R.round16(ties, torch.bfloat16).tolist() == [256.0, 260.0, -256.0, 2048.0, 2048.0, 2048.0]
    assert R.round16(ties, torch.float16).tolist() == [257.0, 259.0, -257.0, 2048.0, 2052.0, 2050.0]
    # integer biases put dyadic sums on such ties
    g = R.gen(2)
    ref = R.dyadic(64, 64, g) @ R.dyadic(64, 64, g).t() + R.ints(64, g)
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        r = R.round16(ref, dt).double()
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - (bits - 1))
        assert ((r - ref).abs() == ulp / 2).any(), dt


def test_padded_views():
    x = R.dyadic(5, 13, R.gen(3))
    for dt, align in ((torch.bfloat16, 8), (torch.float32, 4)):
        v = R.in_nan(x, dt, align, device="cpu")
        assert torch.equal(v.double(), x) and v.stride(0) % align == 0 and v.storage_offset() % align == 0
        base = v._base if v._base is not None else v
        assert torch.isnan(base).sum() == base.numel() - x.numel()
        assert R.f32_vec([v]) == (align % 4 == 0)
        assert not R.f32_vec([R.in_nan(x, dt, align, device="cpu", ld_extra=1)])
        assert not R.f32_vec([R.in_nan(x, dt, align, device="cpu", shift=1)])
    o = R.Out(5, 13, torch.float32, device="cpu")
    o.view.zero_()
    o.assert_sentinels()
    o.buf[1, 3] = 0
    with pytest.raises(AssertionError):
        o.assert_sentinels()
    with pytest.raises(AssertionError):
        R.assert_exact(x.float() + 1e-3, x)
    R.assert_exact(x.bfloat16(), x)


def test_raster_is_a_bijection():
    for tm in range(1, 14):
        for tn in range(1, 14):
            order, _ = R.raster(tm, tn)
            assert sorted(order) == [(i, j) for i in range(tm) for j in range(tn)]


def test_split_properties():
    assert R.split_ranges(3, 2, 2) == [(0, 2), (2, 5)]
    assert "switch_at_t1" in R.split_properties(3, 2, 2)
    assert {"starts_at_KT1", "one_tile_per_split"} <= R.split_properties(1, 1, 2)
    assert "sum8_rounds_2_tail_0" in R.split_properties(8, 8, 16)
    with pytest.raises(AssertionError):
        R.split_properties(1, 0, 2)
