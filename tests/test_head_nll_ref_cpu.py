"""tests/_head_nll_ref.py is the yardstick of the fused head/NLL GPU tests:
here it is proved against fp64 F.linear + F.cross_entropy(reduction="none") +
argmax, and its comparison (``check``) is shown to reject each planted defect
and to accept an fp32 computation of the same quantities."""
import pytest
import torch
import torch.nn.functional as F

import _head_nll_ref as R

IGNORE = -100


def _problem(N=70, H=64, V=21, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, H, generator=g)
    w = torch.randn(V, H, generator=g) / H ** 0.5
    w[V - 2] = w[4]      # an exact tie candidate: columns 4 and V - 2 hold the same row ...
    b = torch.randn(V, generator=g)
    b[V - 2] = b[4]
    labels = torch.randint(0, V, (N,), generator=g)
    labels[::4] = V - 1
    labels[1::7] = IGNORE
    labels[2] = V + 3    # outside the vocabulary: not valid, as in kernels/xent.hip
    h[:10] = 20 * w[4]   # ... and rows 0..9 make them the maximum
    return R.operands(h, w, b, dtype) + (labels,)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, None], ids=["bf16", "fp16", "asis"])
def test_reference_matches_torch_fp64(dtype):
    h64, w64, b64, labels = _problem(dtype=dtype)
    ref = R.reference(h64, w64, b64, labels, IGNORE)
    logits, nll, am, valid = R.torch_reference(h64, w64, b64, labels, IGNORE)
    assert torch.equal(ref["valid"], valid) and not bool(valid[2]) and not bool(valid[1])
    assert torch.allclose(ref["logits"], logits, rtol=0, atol=1e-13)
    assert torch.allclose(ref["nll"], nll, rtol=1e-12, atol=1e-12)
    assert bool((ref["nll"][~valid] == 0).all())
    # the argmax: equal wherever the maximum is unique; on ties the lowest index
    top = ref["logits"].topk(2, dim=-1).values
    unique = top[:, 0] > top[:, 1]
    assert torch.equal(ref["pred"][unique], am[unique])
    assert int((~unique).sum()) >= 10 and bool((ref["pred"][:10] == 4).all())
    acc = ref["accum"]
    assert float(acc[0]) == pytest.approx(float(nll.sum()), rel=1e-12)
    assert float(acc[1]) == float(valid.sum())
    assert float(acc[2]) == float(((ref["pred"] == labels) & valid).sum())
    # the rounding is the operands' only: a 16-bit dtype changes them, None does not
    g = torch.Generator().manual_seed(0)
    assert (dtype is None) == torch.equal(h64[10:].float(), torch.randn(70, 64, generator=g)[10:])


def test_no_bias_and_single_column():
    h64, w64, _, labels = _problem()
    ref = R.reference(h64, w64, None, labels, IGNORE)
    assert torch.allclose(ref["nll"], R.torch_reference(h64, w64, None, labels, IGNORE)[1], rtol=1e-12, atol=1e-12)
    one = R.reference(h64, w64[:1], None, torch.zeros(70, dtype=torch.int64), IGNORE)
    assert bool((one["nll"] == 0).all()) and bool((one["pred"] == 0).all())
    R.check(one["nll"], one["pred"], one)


def test_check_accepts_fp32_arithmetic():
    h64, w64, b64, labels = _problem()
    ref = R.reference(h64, w64, b64, labels, IGNORE)
    logits = F.linear(h64.float(), w64.float(), b64.float())
    lab = torch.where(ref["valid"], labels, torch.full_like(labels, IGNORE))
    nll = F.cross_entropy(logits, lab, ignore_index=IGNORE, reduction="none")
    worst, left = R.check(nll, R.first_argmax(logits), ref, "fp32")
    assert worst < 0.5 and left <= 0.01


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_check_rejects_planted_defect(defect):
    h64, w64, b64, labels = _problem()
    ref = R.reference(h64, w64, b64, labels, IGNORE)
    bad = R.reference(h64, w64, b64, labels, IGNORE, defect=defect)
    R.check(ref["nll"], ref["pred"], ref)  # (the reference passes its own comparison)
    with pytest.raises(AssertionError):
        R.check(bad["nll"], bad["pred"], ref, defect)


def test_check_rejects_16bit_logits():
    """What the fused kernel is for: logits rounded to bf16 before the
    softmax miss the per-row bound."""
    g = torch.Generator().manual_seed(5)
    h = 3 * torch.randn(64, 64, generator=g)
    w = torch.randn(96, 64, generator=g) / 8
    labels = torch.randint(0, 96, (64,), generator=g)
    h64, w64, _ = R.operands(h, w, None, torch.bfloat16)
    ref = R.reference(h64, w64, None, labels, IGNORE)
    rounded = ref["logits"].to(torch.bfloat16).double()
    nll = torch.logsumexp(rounded, -1) - rounded.gather(1, labels[:, None])[:, 0]
    with pytest.raises(AssertionError):
        R.check(nll, ref["pred"], ref)
