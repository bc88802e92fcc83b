"""GPU: the fp32-product GEMM behind ``gemm_f32`` (csrc/kernels/gemm_f32.hip),
``col_sum`` / ``splitk_sum`` and ``ops.gemm.linear`` with its autograd
functions, element by element against the exact result.

Dyadic operands in NaN padding, outputs in sentinels (tests/_gemm_ref.py): an
fp32 result must equal the fp64 CPU value, a 16-bit result its one rounding.
Shapes sit on the kernel's break points (tile width BN at N = 32 / 64, the
128-row tile, the k-tile depth 16 / 32, ragged K with a second segment, empty
splits, the vector and the element-wise load path, the unchecked fast loop);
each case computes from the kernel's own conditions which path it takes and
asserts it.

Ordinary values: randn operands under ``|C - ref| <= (K + S + 1) 2^-23 (|A| |B|)``;
worst error / bound ratio measured on an MI355X: 0.020 unsplit, 0.0072 with
three splits (``test_gemm_f32_randn_within_derived_bound``).
"""
import collections

import pytest
import torch

import _gemm_ref as R
from pytorch_distributed_rnn_amd import _ext

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]
COMBOS = [(dt, akm, bkm) for dt in DTYPES for (akm, bkm) in LAYOUTS]
MS = [1, 127, 128, 129, 300]
NS = [1, 31, 32, 33, 64, 65, 128, 129, 200]
KS = [1, 3, 15, 16, 17, 31, 32, 33, 100]


def _mod():
    mod = _ext.require()
    assert hasattr(mod, "gemm_f32")
    return mod


def _store(x64, km, dtype, **kw):
    return R.in_nan(x64.t() if km else x64, dtype, 4, **kw)


def _run(dtype, akm, bkm, M, N, Ks, seed, vec="on", bias=False, out16=False, splitk=1, out=None, accumulate=False,
         rowsum=False, expect_fast=None):
    """One gemm_f32 call on dyadic operands in NaN padding, checked exactly
    (product, row sums, sentinels).  vec: "on", "stride" (row strides no
    multiple of 4) or "base" (bases one element off)."""
    mod, g = _mod(), R.gen(seed)
    A = [R.dyadic(M, k, g) for k in Ks]
    B = [R.dyadic(N, k, g) for k in Ks]
    ref = sum(a @ b.t() for a, b in zip(A, B))
    pad = {"on": {}, "stride": dict(ld_extra=1), "base": dict(shift=1)}[vec]
    dA, dB = [], []
    for ops, dev, km in ((A, dA, akm), (B, dB, bkm)):
        for x in ops:
            extra = pad.get("ld_extra", 0)
            t = _store(x, km, dtype, ld_extra=extra, shift=pad.get("shift", 0))
            if dev and t.stride(0) == dev[0].stride(0):       # lda2 != lda, ldb2 != ldb
                t = _store(x, km, dtype, ld_extra=extra + 8, shift=pad.get("shift", 0))
            dev.append(t)
    is_vec = R.f32_vec(dA + dB)
    assert is_vec == (vec == "on"), "the padding does not give the load path this case is listed for"
    K2 = Ks[1] if len(Ks) > 1 else 0
    bn, bk, nt = R.f32_plan(dtype, akm, M, N, Ks[0], K2)
    fast, tiles = R.f32_fast_tiles(is_vec, M, N, Ks[0], K2, bn, bk)
    if expect_fast is not None:
        assert (fast, tiles) == expect_fast, (fast, tiles)
    kw = {}
    if K2:
        assert dA[1].stride(0) != dA[0].stride(0) and dB[1].stride(0) != dB[0].stride(0)
        kw.update(A2=dA[1], B2=dB[1])
    if bias:
        b64 = R.ints(N, g)
        ref = ref + b64
        kw["bias"] = b64.float().cuda()
    o = None
    if out is not None:
        base = R.dyadic(M, N, g) * 8 if accumulate else None
        o = R.Out(M, N, dtype if out16 else torch.float32, align=4, pad_cols=(out == "strided"), base64=base)
        if accumulate:
            ref = ref + base
        kw.update(out=o.view, accumulate=accumulate)
    C, rs = mod.gemm_f32(dA[0], akm, dB[0], bkm, out16=out16, splitk=splitk, rowsum=rowsum, **kw)
    what = f"gemm_f32 {dtype} akm={akm} bkm={bkm} {M}x{N}x{Ks} vec={vec} splitk={splitk} BN={bn} BK={bk} nt={nt}"
    assert C.shape == (M, N) and C.dtype == (dtype if out16 else torch.float32)
    if o is not None:
        assert C.data_ptr() == o.view.data_ptr()
        o.assert_sentinels()
    R.assert_exact(C, ref, what)
    if rowsum:
        assert rs.shape == (M,)
        R.assert_exact(rs, sum(a.sum(1) for a in A), what + " rowsum")
    return bn, bk, nt


# ---------------------------------------------------------------- axes: every value with every dtype and layout
AXES = [(dt, akm, bkm, MS[(i + c) % 5], NS[i], KS[(i + 2 * c) % 9])
        for c, (dt, akm, bkm) in enumerate(COMBOS) for i in range(9)]


def test_gemm_f32_axes_cover_every_value_with_every_combo():
    for c in COMBOS:
        mine = [a for a in AXES if a[:3] == c]
        assert {a[3] for a in mine} == set(MS) and {a[4] for a in mine} == set(NS) and {a[5] for a in mine} == set(KS)
    # the break points: BN at N = 32 | 33 and 64 | 65, two tile columns past 128; the 128-row tile; BK 16 and 32
    bns = [R.f32_plan(torch.float32, False, 1, n, 16)[0] for n in (32, 33, 64, 65, 128, 129)]
    assert bns == [32, 64, 64, 128, 128, 128]
    assert [-(-m // 128) for m in (127, 128, 129)] == [1, 1, 2]
    assert [R.f32_plan(torch.float32, True, 1, 1, k)[1:] for k in (31, 32, 33)] == [(32, 1), (32, 1), (32, 2)]
    assert [R.f32_plan(torch.bfloat16, True, 1, 1, k)[1:] for k in (15, 16, 17)] == [(16, 1), (16, 1), (16, 2)]


@pytest.mark.parametrize("dtype,akm,bkm,M,N,K", AXES)
def test_gemm_f32_axes(dtype, akm, bkm, M, N, K):
    _run(dtype, akm, bkm, M, N, [K], seed=M * 7 + N * 3 + K, out="strided", rowsum=True)


# ---------------------------------------------------------------- load paths
@pytest.mark.parametrize("vec", ["stride", "base"])
@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_elementwise_loads(dtype, akm, bkm, vec):
    """vec == 0: every quad is loaded element by element (129 x 65 x 33: ragged in M, N and K)."""
    _run(dtype, akm, bkm, 129, 65, [33], seed=5, vec=vec, expect_fast=(0, 2))


@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_fast_and_checked_loops(dtype, akm, bkm):
    """256 x 128 x 64 aligned: both tiles take the unchecked load_fast loop; one
    more row, column or k sends tiles back to the checked loop."""
    _run(dtype, akm, bkm, 256, 128, [64], seed=6, expect_fast=(2, 2), rowsum=True)
    _run(dtype, akm, bkm, 256, 128, [64, 32], seed=7, expect_fast=(2, 2))
    _run(dtype, akm, bkm, 257, 128, [64], seed=8, expect_fast=(2, 3))
    _run(dtype, akm, bkm, 256, 132, [64], seed=9, expect_fast=(2, 4))
    _run(dtype, akm, bkm, 256, 128, [72], seed=10, expect_fast=(0, 2))
    _run(dtype, akm, bkm, 256, 128, [64], seed=11, vec="stride", expect_fast=(0, 2))


# ---------------------------------------------------------------- second segment after a ragged first
@pytest.mark.parametrize("K1", [17, 32])
@pytest.mark.parametrize("K2", [1, 16, 40])
@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_two_segments(dtype, akm, bkm, K1, K2):
    """129 x 200: two tile rows and two tile columns (row sums only from column 0)."""
    bn, bk, nt = _run(dtype, akm, bkm, 129, 200, [K1, K2], seed=K1 + K2, rowsum=True, out="strided")
    assert bn == 128 and nt == -(-K1 // bk) + -(-K2 // bk)
    if K1 == 17:
        assert K1 % bk        # the first segment's last k-tile is zero-filled before segment 2 starts


# ---------------------------------------------------------------- split-K
@pytest.mark.parametrize("splitk", [2, 8, 9])
@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_splitk(dtype, akm, bkm, splitk):
    """300 x 200 x (100 + 40), row sums per split, with and without accumulate;
    splitk_sum's 8-wide loop at 8 and 8 + 1."""
    bn, bk, nt = _run(dtype, akm, bkm, 300, 200, [100, 40], seed=splitk, splitk=splitk, rowsum=True, out="rows")
    assert nt == (10 if bk == 16 else 6)
    _run(dtype, akm, bkm, 300, 200, [100, 40], seed=splitk + 1, splitk=splitk, rowsum=True, out="rows", accumulate=True)
    _run(dtype, akm, bkm, 300, 200, [100], seed=splitk + 2, splitk=splitk, rowsum=True)


@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_empty_splits_contribute_zeros(dtype, akm, bkm):
    """K = 16, splitk = 3: one k-tile, so two splits run no k-tile at all and
    must write exact zeros (product and row sums)."""
    bn, bk, nt = _run(dtype, akm, bkm, 129, 65, [16], seed=3, splitk=3, rowsum=True, out="rows")
    assert nt == 1
    assert sum(1 for y in range(3) if nt * y // 3 == nt * (y + 1) // 3) == 2


# ---------------------------------------------------------------- epilogue options
@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_epilogue_options(dtype, akm, bkm):
    M, N, K = 129, 65, 33
    _run(dtype, akm, bkm, M, N, [K], seed=21, bias=True, out="strided")
    _run(dtype, akm, bkm, M, N, [K], seed=22, accumulate=True, out="strided", rowsum=True)
    _run(dtype, akm, bkm, M, N, [K], seed=23, bias=True)
    if dtype != torch.float32:
        _run(dtype, akm, bkm, M, N, [K], seed=24, out16=True, bias=True, out="strided")
        _run(dtype, akm, bkm, M, N, [K], seed=25, out16=True)
        _run(dtype, akm, bkm, 300, 200, [100, 17], seed=26, out16=True, bias=True, rowsum=True)


# ---------------------------------------------------------------- col_sum
CS_ROWS = [1, 3, 4, 15, 16, 17, 31, 32, 33, 65, 1000]
CS_COLS = [1, 4, 5, 255, 256, 257, 512, 1024]


@pytest.mark.parametrize("dtype", DTYPES)
def test_col_sum_exact(dtype):
    """Every rows x cols pair, contiguous and as a strided view in NaN padding.
    cols % 512 == 0 with 16-bit input takes the 8-column kernel (rows 31 / 32 /
    33 and 65 / 1000 around its 32-row unroll), anything else the 4-column one
    (16-row unroll)."""
    mod, g = _mod(), R.gen(31)
    for rows in CS_ROWS:
        for cols in CS_COLS:
            x = R.dyadic(rows, cols, g)
            ref = x.sum(0)
            R.assert_exact(mod.col_sum(x.to(dtype).cuda()), ref, f"col_sum {dtype} {rows}x{cols}")
            v = R.in_nan(x, dtype, 8)
            if dtype != torch.float32 and cols % 512 == 0:     # pdrnn_col_sum's condition for the 8-column kernel
                assert v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 0
            R.assert_exact(mod.col_sum(v), ref, f"col_sum {dtype} {rows}x{cols} strided")
            if cols in (5, 512):
                odd = R.in_nan(x, dtype, 4, ld_extra=1)       # element-wise loads of the 4-column kernel
                R.assert_exact(mod.col_sum(odd), ref, f"col_sum {dtype} {rows}x{cols} odd ld")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(33, 512), (1000, 257), (17, 5)])
def test_col_sum_accumulates_into_two_tensors(dtype, rows, cols):
    mod, g = _mod(), R.gen(32)
    x = R.dyadic(rows, cols, g)
    b0, b1 = R.ints(cols, g), R.dyadic(cols, 1, g)[:, 0]
    t0, t1 = b0.float().cuda(), b1.float().cuda()
    r = mod.col_sum(R.in_nan(x, dtype, 8), [t0, t1])
    assert r.data_ptr() == t0.data_ptr()
    R.assert_exact(t0, b0 + x.sum(0), "accumulate_into[0]")
    R.assert_exact(t1, b1 + x.sum(0), "accumulate_into[1]")


# ---------------------------------------------------------------- derived bound, ordinary values
_RATIOS = {}


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("dtype,akm,bkm", COMBOS)
def test_gemm_f32_randn_within_derived_bound(dtype, akm, bkm, splitk):
    """|C - ref| <= (K + S + 1) 2^-23 (|A| |B|), 129 x 65 x 100.  Worst error /
    bound over all layouts on an MI355X: 0.020 for fp32 inputs, 0.0061 for
    16-bit inputs, 0.0072 with three splits."""
    mod = _mod()
    M, N, K = 129, 65, 100
    torch.manual_seed(19)
    A64 = torch.randn(M, K).to(dtype).double()
    B64 = torch.randn(N, K).to(dtype).double()
    C, _ = mod.gemm_f32(_store(A64, akm, dtype), akm, _store(B64, bkm, dtype), bkm, splitk=splitk)
    ratio = R.bound_ratio(C, A64, B64, splitk)
    _RATIOS[splitk] = max(_RATIOS.get(splitk, 0.0), ratio)
    print(f"gemm_f32 bound ratio splitk={splitk} {dtype} akm={akm} bkm={bkm}: {ratio:.4f} "
          f"(worst so far {_RATIOS[splitk]:.4f})")
    assert ratio <= 1.0


# ---------------------------------------------------------------- ops.gemm.linear
class _Counting:
    """The native module with its GEMM entry points counted."""

    def __init__(self, mod):
        self._mod = mod
        self.calls = collections.Counter()

    def __getattr__(self, name):
        attr = getattr(self._mod, name)
        if name not in ("gemm16", "gemm_f32", "col_sum"):
            return attr

        def counted(*a, **k):
            self.calls[name] += 1
            return attr(*a, **k)
        return counted


@pytest.fixture
def counted(monkeypatch):
    from pytorch_distributed_rnn_amd.ops import gemm as G
    proxy = _Counting(_mod())
    n16, nf32 = G._native, G._native_f32
    monkeypatch.setattr(G, "_native", lambda t: proxy if n16(t) is not None else None)
    monkeypatch.setattr(G, "_native_f32", lambda t: proxy if nf32(t) is not None else None)
    return proxy


# (route, x dtype, x shape, N, native calls of one forward + backward with bias)
#   _Linear16: forward on gemm16; dX on gemm16 when N % 64 == 0, dW when the row count % 64 == 0
#   (else those two products fall to the library inside mm_nk16 / mm_kk); db by col_sum
#   _LinearNarrow: forward, dX and dW (+ db as its row sums) on gemm_f32
LINEAR = [
    ("linear16", torch.bfloat16, (128, 128), 136, dict(gemm16=2, col_sum=1)),
    ("linear16", torch.float16, (3, 11, 128), 136, dict(gemm16=1, col_sum=1)),
    ("linear16", torch.bfloat16, (2, 64, 128), 192, dict(gemm16=3, col_sum=1)),
    ("linear16", torch.float16, (128, 64), 192, dict(gemm16=3, col_sum=1)),
    ("narrow", torch.bfloat16, (3, 11, 128), 6, dict(gemm_f32=3)),
    ("narrow", torch.float16, (300, 100), 32, dict(gemm_f32=3)),
    ("narrow", torch.bfloat16, (33, 100), 100, dict(gemm_f32=3)),
    ("narrow", torch.float32, (3, 11, 9), 6, dict(gemm_f32=3)),
    ("narrow", torch.float32, (300, 100), 200, dict(gemm_f32=3)),
    ("narrow", torch.float32, (33, 9), 200, dict(gemm_f32=3)),
    ("narrow", torch.float32, (129, 100), 6, dict(gemm_f32=3)),
    ("library", torch.bfloat16, (33, 100), 136, dict()),
    ("library", torch.float16, (33, 100), 136, dict()),
]


def _linear_case(xdtype, xshape, N, has_bias, seed):
    g = R.gen(seed)
    K = xshape[-1]
    rows = 1
    for s in xshape[:-1]:
        rows *= s
    x64 = R.dyadic(rows, K, g).view(*xshape)
    w64, b64 = R.dyadic(N, K, g), (R.ints(N, g, lim=100) if has_bias else None)
    dy64 = R.dyadic(rows, N, g).view(*xshape[:-1], N)
    xr, wr = x64.clone().requires_grad_(), w64.clone().requires_grad_()
    br = b64.clone().requires_grad_() if has_bias else None
    torch.nn.functional.linear(xr, wr, br).backward(dy64)
    ref = dict(y=torch.nn.functional.linear(x64, w64, b64), dx=xr.grad, dw=wr.grad, db=br.grad if has_bias else None)
    x = x64.to(xdtype).cuda().requires_grad_()
    w = w64.float().cuda().requires_grad_()
    b = b64.float().cuda().requires_grad_() if has_bias else None
    return x, w, b, dy64.to(xdtype).cuda(), ref, g


def _check16(got, ref64, exact, what):
    if got.dtype == torch.float32 or exact:
        R.assert_exact(got, ref64, what)
    else:
        R.assert_within_ulp16(got, ref64, what)


@pytest.mark.parametrize("mode", ["plain", "direct", "direct_no_grad"])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("route,xdtype,xshape,N,calls", LINEAR)
def test_linear_routes_exact(route, xdtype, xshape, N, calls, has_bias, mode, counted):
    """Forward, dx, dW and db of ops.gemm.linear against fp64 autograd of
    F.linear on the same dyadic tensors; which kernels ran; plain delivery,
    direct accumulation into an existing fp32 .grad (same storage, old + exact)
    and direct mode without a .grad (autograd delivers)."""
    from pytorch_distributed_rnn_amd.ops import gemm as G
    from pytorch_distributed_rnn_amd.ops import gradsink
    x, w, b, dy, ref, g = _linear_case(xdtype, xshape, N, has_bias, seed=N + len(xshape))
    params = [p for p in (w, b) if p is not None]
    old = {}
    if mode == "direct":
        for p in params:
            o64 = (R.dyadic(p.numel(), 1, g) * 8).view(p.shape)
            p.grad = o64.float().cuda()
            old[id(p)] = (o64, p.grad, p.grad.data_ptr())
    with gradsink.direct_grads(mode != "plain"):
        y = G.linear(x, w, b)
        y.backward(dy)
    torch.cuda.synchronize()
    want = dict(calls)
    if not has_bias:
        want.pop("col_sum", None)
    assert dict(counted.calls) == want, f"{route}: native calls {dict(counted.calls)}"
    native = route != "library"
    rows = x.numel() // x.shape[-1]
    assert y.dtype == xdtype and y.shape == ref["y"].shape
    _check16(y, ref["y"], native, "y")
    # dX of _Linear16 leaves the kernel for the library when N is no multiple of 64
    _check16(x.grad, ref["dx"], native and (route == "narrow" or N % 64 == 0), "dx")
    for p, key in ((w, "dw"), (b, "db")):
        if p is None:
            continue
        assert p.grad is not None and p.grad.dtype == torch.float32
        exp = ref[key]
        if mode == "direct":
            o64, gt, ptr = old[id(p)]
            assert not native or (p.grad is gt and p.grad.data_ptr() == ptr), \
                f"{key}: .grad replaced, not accumulated in place"
            exp = exp + o64
        if native:
            R.assert_exact(p.grad, exp, f"{key} ({mode}, {rows} rows)")
        else:
            # the library computes these gradients in 16 bits before autograd widens them
            err = (p.grad.cpu().double() - exp).abs()
            assert (err <= R.U16[xdtype] * ref[key].abs()).all(), f"{key} ({mode})"
