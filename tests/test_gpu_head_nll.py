"""The fused vocabulary head + log-softmax + NLL kernel
(csrc/kernels/head_nll.hip) through ops/head_nll.py, against the fp64
reference of tests/_head_nll_ref.py (proved in test_head_nll_ref_cpu.py).

The reference sees the operands as the kernel reads them (16-bit-rounded
matrices, fp32 bias, widened); the bounds are that module's:

    |nll - ref| <= 2 * max_v(2e-5 + 1e-4 |logit_ref_v|) + 1e-5     per row
    pred == fp64 argmax wherever the fp64 top-two gap exceeds twice the logit
    bound (at most 1 % of the rows left out, asserted)

Shapes (N, H, V): a workgroup owns 256 rows, a column pass 256 columns, a W
tile 64 k, an MFMA tile 16 x 16 x 32.

    1,   32,   1     one row, one column, one 32-block (half a W tile)
    15,  64,   5     N, V below a tile
    16,  96,  16     exactly one tile each way, H = a W tile and a half
    17,  1024, 17    one past a tile, the flagship H
    257, 64,  96     one row block + 1, six column tiles (the char-LM test model's V)
    515, 96,  256    two row blocks + 3, one full column pass (the full-pass kernel)
    257, 32,  257    a second column pass of one column (the online rescale)
    515, 64,  1024   four full passes

Worst |nll - ref| / bound, and rows left out of the argmax comparison, measured
on an MI355X when this file was written (`pytest -s` prints them):

    shape             bf16: nll     left out     fp16: nll     left out
    1,   32,   1            0.0000  0.00 %             0.0000  0.00 %
    15,  64,   5            0.0005  0.00 %             0.0005  0.00 %
    16,  96,  16            0.0006  0.00 %             0.0006  0.00 %
    17,  1024, 17           0.0005  0.00 %             0.0011  0.00 %
    257, 64,  96            0.0010  0.00 %             0.0008  0.39 %
    515, 96,  256           0.0008  0.58 %             0.0009  0.19 %
    257, 32,  257           0.0009  0.00 %             0.0009  0.00 %
    515, 64,  1024          0.0010  0.58 %             0.0013  0.58 %

The 25 cases take 3 s.
"""
import functools

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.ops import head_nll as hn

import _gemm_ref as G
import _head_nll_ref as R

pytestmark = pytest.mark.gpu

CASES = [(1, 32, 1), (15, 64, 5), (16, 96, 16), (17, 1024, 17), (257, 64, 96), (515, 96, 256), (257, 32, 257),
         (515, 64, 1024)]
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
SENTINEL = 12288.0  # exact in fp32 and int32
IGNORE = -100


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _problem(N, H, V, cdt, seed=0, ignore_some=True):
    """(h [N, H] cdt, w fp32 master, bias, labels, fp64 reference), shared and never modified."""
    g = torch.Generator().manual_seed(1000 * N + 10 * H + V + seed)
    h = torch.randn(N, H, generator=g).to(cdt)
    w = torch.randn(V, H, generator=g) / H ** 0.5
    b = torch.randn(V, generator=g)
    labels = torch.randint(0, V, (N,), generator=g)
    labels[::3] = V - 1          # the last column, often
    if ignore_some and N > 2:
        labels[1::5] = IGNORE    # some rows ignored
    h64, w64, b64 = R.operands(h, w, b, cdt)
    return h, w, b, labels, R.reference(h64, w64, b64, labels, IGNORE)


def _guarded(n, dtype):
    flat = torch.full((n + 512,), SENTINEL, device=_dev(), dtype=dtype)
    return flat, flat[256:256 + n]


def _assert_guards(*flats):
    for flat in flats:
        assert bool((flat[:256] == SENTINEL).all()) and bool((flat[-256:] == SENTINEL).all()), \
            "a store outside the output buffer"


def _raw(h, w16, b, labels, accum, guarded=False):
    """The binding itself (16-bit weight given), outputs inside guard zones on request."""
    mod = _ext.require()
    N = h.shape[0]
    if not guarded:
        return mod.head_nll(h, w16, b, labels, IGNORE, accum)
    fn, nll = _guarded(N, torch.float32)
    fp, pred = _guarded(N, torch.int32)
    out = mod.head_nll(h, w16, b, labels, IGNORE, accum, row_nll=nll, pred=pred)
    assert out[0].data_ptr() == nll.data_ptr() and out[1].data_ptr() == pred.data_ptr()
    torch.cuda.synchronize()
    _assert_guards(fn, fp)
    return out


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}H{}V{}".format(*c))
def test_shape_grid_against_fp64(case, cdt):
    """Every shape: h a strided view inside a NaN-filled buffer (NaN rows
    above and past N, NaN columns on both sides), outputs between sentinel
    guard zones, some rows ignored, many labels in the last column."""
    N, H, V = case
    h, w, b, labels, ref = _problem(N, H, V, cdt)
    dev = _dev()
    hv = G.in_nan(h.double(), cdt, 8, device=dev)
    assert hv.stride(0) > H
    accum = hn.new_accum(dev)
    nll, pred = _raw(hv, w.to(dev).to(cdt), b.to(dev), labels.to(dev), accum, guarded=True)
    worst, left = R.check(nll, pred, ref, f"N={N} H={H} V={V} {cdt}")
    print(f"\nhead_nll N={N} H={H} V={V} {cdt}: worst nll error / bound {worst:.4f}, argmax rows left out {left:.2%}")
    acc = accum.cpu()
    assert float(acc[1]) == float(ref["accum"][1])
    got_correct = float(((pred.cpu().long() == labels) & ref["valid"]).sum())
    assert float(acc[2]) == got_correct


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_op_contiguous_no_bias_and_shadow(cdt):
    """The op: fp32 master weight through the shadow registry, no bias, a
    [T, B, H] input with [T, B] labels."""
    N, H, V = 257, 64, 96
    h, w, _, labels, _ = _problem(N, H, V, cdt, ignore_some=False)
    dev = _dev()
    wm = w.to(dev).clone()
    h3 = torch.cat([h, h[:7]]).to(dev).view(4, 66, H)
    lab3 = torch.cat([labels, labels[:7]]).view(4, 66)
    h64, w64, _ = R.operands(h3.reshape(-1, H), w, None, cdt)
    ref = R.reference(h64, w64, None, lab3.reshape(-1), IGNORE)
    nll, pred, accum = hn.head_nll(h3, wm, None, lab3.to(dev), IGNORE)
    R.check(nll, pred, ref, "op")
    assert nll.shape == (264,) and pred.dtype == torch.int32 and accum.dtype == torch.float64
    # after an in-place update of the master the op reads the new weight
    with torch.no_grad():
        wm.mul_(-1.0)
    ref2 = R.reference(h64, -w64, None, lab3.reshape(-1), IGNORE)
    nll2, pred2, _ = hn.head_nll(h3, wm, None, lab3.to(dev), IGNORE)
    R.check(nll2, pred2, ref2, "op after a weight update")


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_exact_ties_go_to_the_lowest_index(cdt):
    """Dyadic operands (tests/_gemm_ref.py: every logit exact in fp32) with
    duplicated weight rows: ties inside one 16-column tile (3, 9), across
    tiles (20, 200), across column passes (5, 300 and 700, 1000); the
    duplicated rows are made the row maximum for a share of the rows."""
    N, H, V = 64, 64, 1024
    g = G.gen(7)
    h64 = G.dyadic(N, H, g)
    w64 = G.dyadic(V, H, g)
    pairs = [(3, 9), (20, 200), (5, 300), (700, 1000)]
    for k, (lo, hi) in enumerate(pairs):
        w64[hi] = w64[lo]
    b64 = torch.zeros(V, dtype=torch.float64)
    for lo, hi in pairs:
        b64[lo] = b64[hi] = 64.0
    # row r favours pair r % 4: its h is that pair's weight row, so the product is the largest
    for r in range(N):
        lo, _ = pairs[r % 4]
        h64[r] = w64[lo]
    labels = torch.arange(N) % V
    ref = R.reference(h64, w64, b64, labels, IGNORE)
    tied = (ref["logits"].topk(2, dim=-1).values.diff(dim=-1)[:, 0] == 0)
    assert int(tied.sum()) >= N // 2, "the construction should tie most rows"
    lows = torch.tensor([p[0] for p in pairs])
    assert bool(torch.isin(ref["pred"][tied], lows).all())
    dev = _dev()
    accum = hn.new_accum(dev)
    nll, pred = _raw(h64.to(dev, cdt), w64.to(dev, cdt), b64.to(dev).float(), labels.to(dev), accum)
    R.check(nll, pred, ref, "ties")
    assert torch.equal(pred.cpu().long()[tied], ref["pred"][tied])


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_overflow_guard_and_rescale(cdt):
    """Logits of about +-80 with each row's maximum in the LAST column pass
    (and for other rows in the first, with a larger value later in the same
    pass): exp without the max subtraction overflows, and a wrong rescale of
    the running sum shows in the loss."""
    N, H, V = 40, 64, 1024
    g = torch.Generator().manual_seed(11)
    h = torch.randn(N, H, generator=g).to(cdt)
    w = (torch.randn(V, H, generator=g) / H ** 0.5)
    b = torch.zeros(V)
    h64, w64, _ = R.operands(h, w, None, cdt)
    raw = h64 @ w64.t()
    scale = 60.0 / float(raw.abs().max())
    w = w * scale
    b[V - 3] = 80.0       # the maximum of every row, in the last pass
    b[1] = -80.0
    b[2] = 70.0           # an early large value the later maximum must rescale
    h64, w64, b64 = R.operands(h, w, b, cdt)
    labels = torch.randint(0, V, (N,), generator=g)
    ref = R.reference(h64, w64, b64, labels, IGNORE)
    assert float(ref["logits"].max()) > 75 and float(ref["logits"].min()) < -75
    assert bool((ref["pred"] >= 768).any())
    dev = _dev()
    nll, pred = _raw(h.to(dev), w.to(dev).to(cdt), b.to(dev), labels.to(dev), hn.new_accum(dev))
    R.check(nll, pred, ref, "overflow guard")


@pytest.mark.parametrize("cdt", DTYPES, ids=IDS)
def test_accum_sums_adds_and_reproduces(cdt):
    N, H, V = 515, 96, 256
    h, w, b, labels, ref = _problem(N, H, V, cdt)
    dev = _dev()
    args = (h.to(dev), w.to(dev).to(cdt), b.to(dev), labels.to(dev))
    a1 = hn.new_accum(dev)
    nll, pred = _raw(*args, a1)
    first = a1.clone()
    own = nll.double().sum().item()
    assert abs(float(first[0]) - own) <= 1e-9 * abs(own)
    assert float(first[1]) == float(ref["valid"].sum())
    assert float(first[2]) == float(((pred.cpu().long() == labels) & ref["valid"]).sum())
    nll_b, pred_b = _raw(*args, a1)  # a second call adds
    assert torch.equal(a1[1:], 2 * first[1:]) and abs(float(a1[0]) - 2 * float(first[0])) <= 1e-12 * abs(own)
    a2 = hn.new_accum(dev)
    _raw(*args, a2)                  # two runs are bitwise equal
    assert torch.equal(a2, first) and torch.equal(nll, nll_b) and torch.equal(pred, pred_b)


def test_refusals_take_the_reference_path(monkeypatch):
    dev = _dev()
    assert not hn.supported(64, 96, torch.float32, dev)
    assert not hn.supported(48, 96, torch.bfloat16, dev)
    assert not hn.supported(64, 1025, torch.bfloat16, dev)
    assert hn.supported(64, 1024, torch.bfloat16, dev) and hn.supported(1024, 256, torch.float16, dev)
    g = torch.Generator().manual_seed(3)
    for H, V, dt in ((64, 96, torch.float32), (48, 96, torch.bfloat16), (64, 1025, torch.bfloat16)):
        h = torch.randn(19, H, generator=g).to(dt)
        w = torch.randn(V, H, generator=g) / H ** 0.5
        b = torch.randn(V, generator=g)
        labels = torch.randint(0, V, (19,), generator=g)
        labels[4] = IGNORE
        monkeypatch.setenv("PDRNN_KERNELS", "hip")
        with pytest.warns(RuntimeWarning, match="head_nll"):
            _ext._WARNED.clear()
            nll, pred, accum = hn.head_nll(h.to(dev), w.to(dev), b.to(dev), labels.to(dev), IGNORE)
        h64, w64, b64 = R.operands(h, w, b, None)
        ref = R.reference(h64, w64, b64, labels, IGNORE)
        assert torch.allclose(nll.cpu().double(), ref["nll"], atol=1e-4, rtol=1e-5)
        assert float(accum[1]) == 18.0
        monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
        with pytest.raises(RuntimeError, match="head_nll"):
            hn.head_nll(h.to(dev), w.to(dev), b.to(dev), labels.to(dev), IGNORE)
