"""fp64 reference of the fused vocabulary head + log-softmax + NLL kernel
(csrc/kernels/head_nll.hip) and the comparison the GPU tests make with it.

``reference`` takes the operands exactly as the kernel reads them -- ``h`` and
the weight rounded through the 16-bit dtype, the bias in fp32, all widened to
fp64 -- so what is left to differ is the kernel's own fp32 arithmetic.  It is
plain ``F.linear`` + ``F.cross_entropy(reduction="none")`` + first-index argmax
semantics and is proved against those in fp64 by test_head_nll_ref_cpu.py, which
also plants each ``defect`` below and shows ``check`` rejecting it.

Bounds (``check``):

* per row ``|nll - ref| <= 2 * max_v(2e-5 + 1e-4 |logit_ref_v|) + 1e-5``: the
  project's per-element bound for fp32 results (tests/_decode_ref.py:bound with
  r = 0) applied to the logits, doubled because log-sum-exp and the target
  logit each move by at most the largest logit error, plus 1e-5 of slack for
  fp32 exp / log;
* ``pred`` equals the fp64 argmax (the lowest index on ties) on every row whose
  fp64 top-two gap exceeds twice that logit bound, or is exactly zero (a true
  tie: the kernel's two logits are then the same fp32 sum of the same terms
  only when the tied columns hold identical operands, which is how the tests
  make ties); at most 1 % of the rows may be left out.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64

DEFECTS = ("no_bias", "next_label", "pad_in_sum", "ties_high")


def operands(h, w, bias, dtype):
    """(h, w, bias) in fp64 on the CPU as the kernel reads them: the matrices
    rounded through ``dtype`` (None: as they are), the bias through fp32."""
    def mat(x):
        x = x.detach().cpu()
        return (x.to(dtype) if dtype is not None else x).to(F64)
    return mat(h), mat(w), (bias.detach().cpu().float().to(F64) if bias is not None else None)


def first_argmax(x):
    V = x.shape[-1]
    idx = torch.arange(V).expand_as(x)
    top = x.max(dim=-1, keepdim=True).values
    return torch.where(x == top, idx, V).min(dim=-1).values


def last_argmax(x):
    V = x.shape[-1]
    idx = torch.arange(V).expand_as(x)
    top = x.max(dim=-1, keepdim=True).values
    return torch.where(x == top, idx, -1).max(dim=-1).values


def reference(h64, w64, b64, labels, ignore_index=-100, defect=None):
    """h64 [N, H], w64 [V, H], b64 [V] or None, labels [N] int64 -> dict of
    logits [N, V], nll [N] (0 on rows that are not valid), pred [N], valid [N]
    and accum [3] = [sum nll, n_valid, n_correct], all fp64 / int64 on the CPU.

    ``defect`` plants one fault a fused kernel could have: the bias dropped; a
    row's label taken from the next row; the zero-valued padding columns (V
    rounded up to the 16-column tile) counted in the sum of exponentials; ties
    going to the highest index."""
    assert defect is None or defect in DEFECTS
    labels = labels.detach().cpu().to(torch.int64)
    N, V = h64.shape[0], w64.shape[0]
    logits = h64 @ w64.t()
    if b64 is not None and defect != "no_bias":
        logits = logits + b64
    if defect == "next_label":
        labels = torch.roll(labels, -1)
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    lse = torch.logsumexp(logits, dim=-1)
    if defect == "pad_in_sum":
        pad = -(-V // 16) * 16 - V
        lse = torch.logsumexp(torch.cat([logits, torch.zeros(N, pad, dtype=F64)], 1), dim=-1)
    tgt = logits.gather(1, torch.where(valid, labels, torch.zeros_like(labels))[:, None])[:, 0]
    nll = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    pred = last_argmax(logits) if defect == "ties_high" else first_argmax(logits)
    accum = torch.stack([nll.sum(), valid.sum().to(F64), ((pred == labels) & valid).sum().to(F64)])
    return {"logits": logits, "nll": nll, "pred": pred, "valid": valid, "accum": accum}


def logit_bound(logits):
    """The per-element fp32 bound of tests/_decode_ref.py (r = 0)."""
    return 2e-5 + 1e-4 * logits.abs()


def nll_bound(ref):
    return 2 * logit_bound(ref["logits"]).max(dim=-1).values + 1e-5


def decided(ref):
    """Rows whose argmax the bound decides: the fp64 top-two gap is above
    twice the row's logit bound, or the top two are exactly equal."""
    logits = ref["logits"]
    if logits.shape[1] == 1:
        return torch.ones(logits.shape[0], dtype=torch.bool)
    top = logits.topk(2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    return (gap > 2 * logit_bound(logits).max(dim=-1).values) | (gap == 0)


def check(row_nll, pred, ref, what=""):
    """Assert the bounds of this module's docstring; returns (worst nll error
    / bound, fraction of rows left out of the argmax comparison)."""
    nll = row_nll.detach().cpu().to(F64)
    pred = pred.detach().cpu().to(torch.int64)
    assert torch.isfinite(nll).all(), f"{what}: a loss that is not finite"
    ratio = (nll - ref["nll"]).abs() / nll_bound(ref)
    worst = float(ratio.max())
    row = int(ratio.argmax())
    assert worst <= 1.0, (f"{what}: row {row}: nll {float(nll[row])!r} vs {float(ref['nll'][row])!r}, "
                          f"{worst:.3f} of the bound")
    assert bool(((nll == 0) | ref["valid"]).all()), f"{what}: a row that is not valid has a loss"
    sure = decided(ref)
    left_out = 1.0 - float(sure.double().mean())
    assert left_out <= 0.01, f"{what}: {left_out:.2%} of the rows are too close to call"
    bad = (sure & (pred != ref["pred"])).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} predictions differ, first at row {int(bad[0])}: "
                              f"{int(pred[bad[0]])} vs {int(ref['pred'][bad[0]])}")
    assert bool(((pred >= 0) & (pred < ref["logits"].shape[1])).all()), f"{what}: a prediction outside the vocabulary"
    return worst, left_out


def torch_reference(h64, w64, b64, labels, ignore_index=-100):
    """The same quantities from F.linear + F.cross_entropy + argmax in fp64
    (labels outside the vocabulary are not accepted by F.cross_entropy: rows
    that are not valid are given the ignore index)."""
    labels = labels.detach().cpu().to(torch.int64)
    V = w64.shape[0]
    logits = F.linear(h64, w64, b64)
    valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
    nll = F.cross_entropy(logits, torch.where(valid, labels, torch.full_like(labels, ignore_index)),
                          ignore_index=ignore_index, reduction="none")
    return logits, nll, logits.argmax(dim=-1), valid
