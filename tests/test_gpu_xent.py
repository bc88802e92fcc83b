"""Fused softmax cross-entropy (csrc/kernels/xent.hip) against F.cross_entropy
in fp64 on the widened stored logits: all three logit dtypes, the 16-bit
gradient writers, strided rows, class counts around one wave, more rows than
partial blocks, argmax ties, ignored rows.

The gradient is compared as ``grad * n_valid`` (softmax - onehot, of order 1)
so that the bound means the same at every N.  Each comparison prints its
worst error as a fraction of its tolerance (``RATIO <quantity> <value>``; run
with ``-s`` to see them).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LOSS_RTOL, LOSS_ATOL = 2e-6, 1e-7
GRAD_ATOL = 2e-6  # on grad * n_valid

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(37, 1000, 3), (37, 1000, 30), (5, 1, 3), (3, 2, 3), (130, 63, 3), (130, 64, 10), (130, 65, 3),
          (70000, 6, 3), (64, 4097, 3), (0, 6, 3)]


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.require()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _assert_rounded(got, g32, dtype, exact=None):
    """``got`` is the fp32 tensor rounded to nearest even in ``dtype``, bit for
    bit.  ``exact`` (fp64, the unrounded product the fp32 value came from):
    where given, an element may instead be that product rounded ONCE -- the
    fp16 writer is one fused multiply-convert (v_fma_mixlo_f16), which differs
    from rounding twice only where the fp32 product sits exactly on an fp16 tie."""
    got, g32 = got.detach().cpu(), g32.detach().cpu()
    want = g32.to(dtype)
    bad = _bits(got) != _bits(want)
    if exact is not None and dtype == torch.float16:
        once = torch.from_numpy(exact.detach().cpu().numpy().astype(np.float16))
        bad &= _bits(got) != _bits(once)
    bad = bad.flatten()
    if bad.any():
        i = bad.nonzero().flatten()[:8]
        rows = [f"{g32.flatten()[k].item():.9e}: got {got.flatten()[k].item():.6e} ({_bits(got).flatten()[k].item() & 0xffff:#06x})"
                f" want {want.flatten()[k].item():.6e} ({_bits(want).flatten()[k].item() & 0xffff:#06x})" for k in i.tolist()]
        raise AssertionError(f"{dtype}: {int(bad.sum())} of {bad.numel()} elements are not the RNE rounding of the "
                             "fp32 gradient:\n" + "\n".join(rows))


def _case(N, C, scale, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * N + C)
    logits = (torch.randn(N, C, generator=g) * scale).to(dtype)
    labels = torch.randint(0, C, (N,), generator=g)
    if N >= 2:
        labels[::7] = -100
    return logits, labels


def _reference(logits, labels):
    """(loss, n_valid, first-index argmax hits, d loss / d logits) in fp64 from
    the stored values."""
    x = logits.double().cpu().requires_grad_()
    loss = F.cross_entropy(x, labels, ignore_index=-100)
    loss.backward()
    valid = labels != -100
    xd = x.detach()
    cols = torch.arange(xd.shape[1]).expand_as(xd)
    first = torch.where(xd == xd.amax(1, keepdim=True), cols, xd.shape[1]).amin(1)
    return loss.item(), int(valid.sum()), int(((first == labels) & valid).sum()), x.grad


def _check_loss(got, ref):
    r = abs(got - ref) / (LOSS_ATOL + LOSS_RTOL * abs(ref))
    print(f"RATIO xent.loss {r:.4f}")
    assert r <= 1.0, f"loss {got} vs {ref}: {r:.3f} x (rtol 2e-6, atol 1e-7)"


def _check_grad(got, ref, n_valid, upstream=1.0):
    err = ((got.double().cpu() - upstream * ref) * (n_valid / upstream)).abs().max().item()
    print(f"RATIO xent.grad {err / GRAD_ATOL:.4f}")
    assert err <= GRAD_ATOL, f"grad * n_valid off by {err:.3e} (> 2e-6)"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N,C,scale", SHAPES)
def test_xent_shapes_and_dtypes(N, C, scale, dtype):
    """Loss, counts and gradient.  A 16-bit head gets its gradient in its own
    dtype, which cannot hold softmax - onehot to 2e-6: there the kernel's fp32
    gradient (xent_bwd's fp32 writer on the same saved values) meets the bound
    and the returned 16-bit gradient is that one rounded to nearest even, bit
    for bit -- together no weaker than the bound on the returned tensor.
    (fp16 at (70000, 6): one element of 420000 is the unrounded product rounded
    once, 0x8117 where the fp32 value -1.659989357e-05 is the tie below it.)"""
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    logits, labels = _case(N, C, scale, dtype)
    lg = logits.cuda().requires_grad_()
    loss, stats = cross_entropy_with_stats(lg, labels.cuda(), -100)
    loss.backward()
    torch.cuda.synchronize()  # no launch error, N == 0 included
    assert lg.grad.dtype == dtype and lg.grad.shape == (N, C)
    if N == 0:
        assert math.isnan(loss.item()) and stats[1].item() == 0 and stats[2].item() == 0
        assert lg.grad.numel() == 0
        return
    ref_loss, n_valid, n_correct, ref_grad = _reference(logits, labels)
    _check_loss(loss.item(), ref_loss)
    assert stats[0].item() == loss.item()
    assert stats[1].item() == n_valid
    assert stats[2].item() == n_correct
    if dtype == torch.float32:
        _check_grad(lg.grad, ref_grad, n_valid)
        return
    st, dl = _mod().xent_fwd(lg.detach(), labels.cuda(), -100, True)
    g32 = _mod().xent_bwd(dl, torch.ones(1, device="cuda"), st, torch.float32)
    assert g32.dtype == torch.float32
    _check_grad(g32, ref_grad, n_valid)
    scale = np.float32(1.0) / np.float32(n_valid)  # grad_out / n_valid as the kernel forms it
    _assert_rounded(lg.grad, g32, dtype, exact=dl.double() * float(scale))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_xent_strided_rows_are_bitwise_the_contiguous_result(dtype):
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    N, C = 130, 65
    g = torch.Generator().manual_seed(5)
    big = (torch.randn(N, C + 5, generator=g) * 3).to(dtype).cuda().requires_grad_()
    labels = torch.randint(0, C, (N,), generator=g)
    labels[::7] = -100
    view = big[:, 2:2 + C]
    assert view.stride() == (C + 5, 1) and not view.is_contiguous()
    loss_v, stats_v = cross_entropy_with_stats(view, labels.cuda(), -100)
    loss_v.backward()
    cont = big.detach()[:, 2:2 + C].contiguous().requires_grad_()
    loss_c, stats_c = cross_entropy_with_stats(cont, labels.cuda(), -100)
    loss_c.backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(stats_v), _bits(stats_c))
    assert torch.equal(_bits(big.grad[:, 2:2 + C].contiguous()), _bits(cont.grad))
    assert cont.grad.abs().max().item() > 0
    assert big.grad[:, :2].abs().max().item() == 0 and big.grad[:, 2 + C:].abs().max().item() == 0
    ref_loss, n_valid, n_correct, _ = _reference(cont.detach().cpu(), labels)
    _check_loss(loss_v.item(), ref_loss)
    assert stats_v[1].item() == n_valid and stats_v[2].item() == n_correct


def test_xent_upstream_scale():
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    logits, labels = _case(130, 65, 3, torch.float32, seed=9)
    lg = logits.cuda().requires_grad_()
    loss, _ = cross_entropy_with_stats(lg, labels.cuda(), -100)
    (3.5 * loss).backward()
    _, n_valid, _, ref_grad = _reference(logits, labels)
    _check_grad(lg.grad, ref_grad, n_valid, upstream=3.5)


def test_xent_bwd_16bit_writers_round_to_nearest_even():
    """One saved softmax - onehot through all three writers of xent_bwd: the
    bf16 / fp16 outputs are the fp32 output rounded to nearest even, bit for
    bit -- at (4096, 256) a good part of the fp16 values is subnormal.  (No
    fp32 value of this case sits on an fp16 tie, see _assert_rounded.)"""
    N, C = 4096, 256
    logits, labels = _case(N, C, 3, torch.float32, seed=3)
    mod = _mod()
    st, dl = mod.xent_fwd(logits.cuda(), labels.cuda(), -100, True)
    one = torch.ones(1, device="cuda")
    g32 = mod.xent_bwd(dl, one, st, torch.float32)
    assert g32.dtype == torch.float32 and torch.isfinite(g32).all()
    _, n_valid, _, ref_grad = _reference(logits, labels)
    _check_grad(g32, ref_grad, n_valid)
    for dtype in (torch.bfloat16, torch.float16):
        got = mod.xent_bwd(dl, one, st, dtype)
        assert got.dtype == dtype
        want = g32.cpu().to(dtype)
        if dtype == torch.float16:
            sub = (want != 0) & (want.float().abs() < 2.0 ** -14)
            assert sub.float().mean().item() >= 0.01, "no fp16 subnormals in this case"
        _assert_rounded(got, g32, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_xent_bwd_writers_on_special_values(dtype):
    """Upstream gradient 1 and one valid row (scale exactly 1): every writer of
    xent_bwd returns its source rounded once -- rounding ties both ways, the
    edges of the 16-bit ranges, fp16 subnormals, signed zeros and infinities
    bit for bit, and a NaN of any bit pattern (0x7fffffff and 0xffffffff, which
    an unguarded ``u + 0x7fff`` turns into -0 and +0, and 0x7f800001) stays a
    NaN.  The table holds no fp32 subnormal."""
    import _embedding_ref as E
    src = E.special_values()
    b = E.special_bits()
    for nan in (0x7fffffff, 0xffffffff, 0x7f800001):
        assert torch.isnan(src[(b == nan).nonzero()[0, 0]])
    src = src.repeat(5).view(5, -1)   # more than one block of 256
    stats = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    got = _mod().xent_bwd(src.cuda(), torch.ones(1, device="cuda"), stats, dtype)
    assert got.dtype == dtype and got.shape == src.shape
    E.assert_bits(got, src.to(dtype), str(dtype))


def test_xent_argmax_ties_take_the_first_index():
    """The maximum at two columns: the lower column is the prediction --
    columns 3 and 67 meet in one lane's strided loop, 3 and 10 in the wave
    reduction, 5 and 64 there with the lower column in the higher lane."""
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    C = 130
    pairs = [(3, 67), (3, 10), (5, 64)]
    g = torch.Generator().manual_seed(11)
    rows, labels = [], []
    for a, b in pairs:
        for label in (a, b):
            x = torch.randn(C, generator=g).clamp_(-3, 3)
            x[a] = x[b] = 5.0
            rows.append(x)
            labels.append(label)
    expected = len(pairs)  # first-index rule: the rows labelled with the lower column
    for dtype in DTYPES:
        logits = torch.stack(rows).to(dtype).cuda()
        _, stats = cross_entropy_with_stats(logits, torch.tensor(labels).cuda(), -100)
        assert stats[1].item() == len(rows)
        assert stats[2].item() == expected, dtype


def test_xent_nan_logit_gives_nan_loss():
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    logits, labels = _case(37, 100, 3, torch.float32, seed=13)
    logits[5, 70] = float("nan")
    assert labels[5] != -100
    loss, stats = cross_entropy_with_stats(logits.cuda(), labels.cuda(), -100)
    assert math.isnan(F.cross_entropy(logits.double(), labels, ignore_index=-100).item())
    assert math.isnan(loss.item())
    assert stats[1].item() == int((labels != -100).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_xent_all_rows_ignored_has_zero_gradient(dtype):
    """No valid row: NaN loss and a ZERO gradient, as F.cross_entropy gives
    (the saved softmax - onehot is all 0; scaling it by 1 / n_valid = inf
    made every logit gradient NaN)."""
    from pytorch_distributed_rnn_amd.ops.xent import cross_entropy_with_stats
    logits, _ = _case(37, 10, 3, dtype)
    labels = torch.full((37,), -100)
    x = logits.double().requires_grad_()
    ref = F.cross_entropy(x, labels, ignore_index=-100)
    ref.backward()
    assert math.isnan(ref.item()) and x.grad.abs().max().item() == 0
    lg = logits.cuda().requires_grad_()
    loss, stats = cross_entropy_with_stats(lg, labels.cuda(), -100)
    loss.backward()
    assert math.isnan(loss.item()) and stats[1].item() == 0 and stats[2].item() == 0
    assert lg.grad.dtype == dtype
    assert torch.equal(lg.grad.float().cpu(), torch.zeros(37, 10))
