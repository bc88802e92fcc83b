"""GPU: the 256 x 256 x 64 ping-pong GEMM behind ``gemm16`` (csrc/kernels/gemm.hip,
csrc/include/pdrnn/gemm_pp.h) and ``splitk_sum``, element by element against the
exact product.

Operands are dyadic (tests/_gemm_ref.py): every product and every partial sum
is exact in fp32 in any order, so an fp32 output must ``torch.equal`` the fp64
CPU matmul and a 16-bit output its one round-to-nearest-even -- a dropped,
doubled or mis-paired product, a tile computed twice or never, a swapped lane
of the 16-bit pack or a K-tile read from the wrong segment changes at least
one element.  Operands sit inside NaN padding and outputs inside sentinels.
What a case is listed for (K-tile count, raster group sizes, where a split
starts, where the segment switch falls) is computed with the kernel's integer
arithmetic and asserted, not trusted from the shape list.

Ordinary values (section "derived bound"): randn operands against the fp64
product under ``|C - ref| <= (K + S + 1) 2^-23 (|A| |B|)`` (+ ``u16 |ref|`` for a
16-bit output).  Worst error / bound ratio measured on an MI355X: 0.0024 for
an fp32 output, 0.0013 with three splits, 0.93 for a 16-bit output (details in
``test_gemm16_randn_within_derived_bound``).
"""
import pytest
import torch

import _gemm_ref as R
from pytorch_distributed_rnn_amd import _ext

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]   # (A k-major, B k-major)
TILE = 256


def _mod():
    mod = _ext.require()
    assert hasattr(mod, "gemm16")
    return mod


def _store(x64, km, dtype, ld_extra=0):
    """logical [rows, K] operand -> padded device storage ([K, rows] when k-major)."""
    return R.in_nan(x64.t() if km else x64, dtype, 8, ld_extra=ld_extra)


def _run(dtype, akm, bkm, M, N, Ks, seed, out16=False, bias=False, splitk=1, out=None, accumulate=False):
    """One gemm16 call on dyadic operands in NaN padding; ``out``: None, "rows"
    (contiguous, sentinel rows) or "strided" (sentinel rows and columns).
    Checks the result exactly and every sentinel."""
    assert R.gemm16_supported(M, N, Ks[0], Ks[1] if len(Ks) > 1 else 0, akm, bkm, out16, splitk, accumulate), \
        "the case list holds a shape the kernel refuses"
    assert sum(Ks) <= R.K_MAX
    mod, g = _mod(), R.gen(seed)
    A = [R.dyadic(M, k, g) for k in Ks]
    B = [R.dyadic(N, k, g) for k in Ks]
    ref = sum(a @ b.t() for a, b in zip(A, B))
    dA = [_store(a, akm, dtype, ld_extra=8 * i) for i, a in enumerate(A)]       # lda2 != lda, ldb2 != ldb
    dB = [_store(b, bkm, dtype, ld_extra=16 * i) for i, b in enumerate(B)]
    kw = {}
    if len(Ks) > 1:
        assert dA[1].stride(0) != dA[0].stride(0) and dB[1].stride(0) != dB[0].stride(0)
        kw.update(A2=dA[1], B2=dB[1])
    if bias:
        b64 = R.ints(N, g)
        ref = ref + b64
        kw["bias"] = b64.float().cuda()
    o = None
    if out is not None:
        base = R.dyadic(M, N, g) * 8 if accumulate else None      # integers up to +-16
        o = R.Out(M, N, dtype if out16 else torch.float32, pad_cols=(out == "strided"), base64=base)
        if accumulate:
            ref = ref + base
        kw.update(out=o.view, accumulate=accumulate)
    C = mod.gemm16(dA[0], akm, dB[0], bkm, out16=out16, splitk=splitk, **kw)
    assert C.shape == (M, N) and C.dtype == (dtype if out16 else torch.float32)
    if o is not None:
        assert C.data_ptr() == o.view.data_ptr()
        o.assert_sentinels()
    R.assert_exact(C, ref, f"gemm16 {dtype} akm={akm} bkm={bkm} {M}x{N}x{Ks} out16={out16} splitk={splitk}")


# ---------------------------------------------------------------- K-tile counts
# 264 x 136: two tile-rows (the second ragged), one tile-column, N no multiple of 64.
# KT = 1 takes the short prologue wait, KT = 2 has no steady-state tile (more2
# never true), KT = 3 exactly one, 4 and 5 refill both LDS slots.
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("akm,bkm", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320])
def test_gemm16_ktile_counts(K, dtype, akm, bkm, out16):
    assert K // 64 in (1, 2, 3, 4, 5) and -(-264 // TILE) == 2 and -(-136 // TILE) == 1
    _run(dtype, akm, bkm, 264, 136, [K], seed=K + out16, out16=out16, bias=out16, out="strided")


# ---------------------------------------------------------------- tile edges, K = 64
EDGE_SHAPES = [(8, 8), (9, 8), (255, 257), (256, 256), (264, 248), (248, 264)]
EDGE_CASES = [(M, N, akm, bkm, out16) for (M, N) in EDGE_SHAPES for (akm, bkm) in LAYOUTS for out16 in (False, True)
              if R.gemm16_supported(M, N, 64, 0, akm, bkm, out16)]


def test_gemm16_tile_edge_case_list():
    got = {(M, N): sorted({(a, b) for (m, n, a, b, _) in EDGE_CASES if (m, n) == (M, N)}) for M, N in EDGE_SHAPES}
    assert got[(9, 8)] == [(False, False), (False, True)]          # M % 8: A row-major only
    assert got[(255, 257)] == [(False, False)]                     # N % 8 as well: B row-major only, fp32 out
    assert all(len(got[s]) == 4 for s in EDGE_SHAPES if s not in ((9, 8), (255, 257)))
    assert not any(o for (M, N, _, _, o) in EDGE_CASES if N % 8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,akm,bkm,out16", EDGE_CASES)
def test_gemm16_tile_edges(M, N, akm, bkm, out16, dtype):
    _run(dtype, akm, bkm, M, N, [64], seed=M * 3 + N, out16=out16, bias=out16, out="strided")


# ---------------------------------------------------------------- tile raster
# (M, N, tiles_m, tiles_n, group sizes used, nwg & 7)
RASTER = [
    (1288, 520, 6, 3, {4, 2}, 2),     # short last group of 2, 18 tiles over 8 XCD runs of 3 / 2
    (1032, 8, 5, 1, {4, 1}, 5),       # fewer workgroups than XCDs
    (2056, 8, 9, 1, {4, 1}, 1),       # nwg = 9
    (520, 2056, 3, 9, {3}, 3),        # a single short group, 27 tiles
]


@pytest.mark.parametrize("dtype,akm,bkm", [(torch.bfloat16, False, False), (torch.float16, True, True)])
@pytest.mark.parametrize("M,N,tiles_m,tiles_n,sizes,r8", RASTER)
def test_gemm16_raster(M, N, tiles_m, tiles_n, sizes, r8, dtype, akm, bkm):
    assert (-(-M // TILE), -(-N // TILE)) == (tiles_m, tiles_n)
    order, used = R.raster(tiles_m, tiles_n, group=4)   # the product build's raster groups 4 tile-rows
    assert used == sizes and (tiles_m * tiles_n) & 7 == r8
    assert sorted(order) == [(i, j) for i in range(tiles_m) for j in range(tiles_n)]
    _run(dtype, akm, bkm, M, N, [64], seed=M + N, out="strided")


# ---------------------------------------------------------------- two K segments, one split
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K1,K2", [(64, 64), (64, 128), (128, 64), (192, 192)])
def test_gemm16_two_segments(K1, K2, dtype):
    # (64, *): the switch is issued from the prologue (t = 1); (128, 64): at t = 2, the
    # first steady-state refill; (192, 192): at t = 3 with three more tiles behind it
    _run(dtype, False, True, 264, 136, [K1, K2], seed=K1 + 2 * K2, out16=True, out="strided")        # dX
    _run(dtype, True, True, 264, 136, [K1, K2], seed=K1 + 2 * K2 + 1, out="strided")                 # dW
    _run(dtype, True, True, 264, 136, [K1, K2], seed=K1 + 2 * K2 + 2, out="strided", accumulate=True)


# ---------------------------------------------------------------- split-K across the segment boundary
# With KTALL = KT1 + KT2 K-tiles, split y of S takes [KTALL y / S, KTALL (y + 1) / S):
#   (1, 1, 2)  [0,1) [1,2)              one tile each; split 1 starts at KT1
#   (2, 3, 2)  [0,2) [2,5)              split 1 starts exactly at KT1
#   (3, 2, 2)  [0,2) [2,5)              split 1 switches at t = 1 (issued from its prologue)
#   (4, 3, 3)  [0,2) [2,4) [4,7)        two splits inside segment 1, the last starts at KT1
#   (3, 4, 2)  [0,3) [3,7)              split 1 starts exactly at KT1
#   (5, 2, 2)  [0,3) [3,7)              split 1 switches at t = 2
#   (1, 6, 7)  one tile each; split 1 starts at KT1
#   (7, 3, 8)  sizes 1 1 1 2 1 1 1 2; split 6 = [7,8) starts at KT1; splitk_sum's 8-wide loop once
#   (9, 0, 9)  one tile each, one segment; 8 + 1 partials
#   (8, 8, 16) one tile each; split 8 starts at KT1; two rounds of the 8-wide loop
SPLITS = [
    (1, 1, 2, {"one_tile_per_split", "starts_at_KT1"}),
    (2, 3, 2, {"starts_at_KT1"}),
    (3, 2, 2, {"switch_at_t1"}),
    (4, 3, 3, {"inside_segment1", "starts_at_KT1"}),
    (3, 4, 2, {"starts_at_KT1"}),
    (5, 2, 2, {"switch_at_t2"}),
    (1, 6, 7, {"one_tile_per_split", "starts_at_KT1"}),
    (7, 3, 8, {"one_tile_split", "two_tile_split", "starts_at_KT1", "sum8_rounds_1_tail_0"}),
    (9, 0, 9, {"one_tile_per_split", "sum8_rounds_1_tail_1"}),
    (8, 8, 16, {"one_tile_per_split", "starts_at_KT1", "sum8_rounds_2_tail_0"}),
]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KT1,KT2,S,props", SPLITS)
def test_gemm16_splitk_segments(KT1, KT2, S, props, dtype, accumulate):
    assert props <= R.split_properties(KT1, KT2, S), (props, R.split_properties(KT1, KT2, S))
    Ks = [64 * KT1] + ([64 * KT2] if KT2 else [])
    _run(dtype, True, True, 264, 520, Ks, seed=100 * KT1 + 10 * KT2 + S, splitk=S, out="rows", accumulate=accumulate)


def test_gemm16_splitk_list_covers_every_edge():
    allp = set().union(*(R.split_properties(a, b, s) for a, b, s, _ in SPLITS))
    assert {"one_tile_per_split", "starts_at_KT1", "switch_at_t1", "switch_at_t2", "inside_segment1", "two_tile_split",
            "sum8_rounds_1_tail_0", "sum8_rounds_1_tail_1", "sum8_rounds_2_tail_0", "sum8_rounds_0_tail_2"} <= allp


# ---------------------------------------------------------------- 16-bit epilogue
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("out", [None, "strided"])
@pytest.mark.parametrize("akm,bkm", [(False, False), (False, True)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [8, 72, 264])
def test_gemm16_out16_chunk_guard(N, dtype, akm, bkm, out, bias):
    # N = 8: one 16-byte chunk of wave column 0; 72: one chunk into wave column 1;
    # 264: one chunk into the second tile column.  264 rows: both wave rows and a ragged tile-row.
    assert N % 64 == 8
    _run(dtype, akm, bkm, 264, N, [64], seed=N + bias, out16=True, bias=bias, out=out)


# ---------------------------------------------------------------- refusals (host checks, nothing is launched)
def _z(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def test_gemm16_refusals():
    mod = _mod()
    ok = mod.gemm16(_z(16, 64), False, _z(16, 64), False)          # the well-formed neighbour of every case below
    assert ok.shape == (16, 16)
    with pytest.raises(RuntimeError):      # K % 64
        mod.gemm16(_z(16, 96), False, _z(16, 96), False)
    with pytest.raises(RuntimeError):      # k-major A, M % 8
        mod.gemm16(_z(64, 16)[:, :12], True, _z(16, 64), False)
    with pytest.raises(RuntimeError):      # k-major B, N % 8
        mod.gemm16(_z(16, 64), False, _z(64, 16)[:, :12], True)
    with pytest.raises(RuntimeError):      # 16-bit out, N % 8
        mod.gemm16(_z(16, 64), False, _z(12, 64), False, out16=True)
    with pytest.raises(RuntimeError):      # row stride % 8
        mod.gemm16(_z(16, 68)[:, :64], False, _z(16, 64), False)
    with pytest.raises(RuntimeError):      # base not 16-byte aligned
        mod.gemm16(_z(16, 72)[:, 4:68], False, _z(16, 64), False)
    with pytest.raises(RuntimeError):      # the same for a second-segment operand
        mod.gemm16(_z(16, 64), False, _z(16, 64), False, A2=_z(16, 72)[:, 4:68], B2=_z(16, 64))
    with pytest.raises(RuntimeError):      # split-K with a 16-bit output
        mod.gemm16(_z(16, 128), False, _z(16, 128), False, out16=True, splitk=2)
    with pytest.raises(RuntimeError):      # more splits than K-tiles
        mod.gemm16(_z(16, 128), False, _z(16, 128), False, splitk=3)
    with pytest.raises(RuntimeError):      # segment 2 not in whole K-tiles
        mod.gemm16(_z(16, 64), False, _z(16, 64), False, A2=_z(16, 32), B2=_z(16, 32))
    assert not mod.gemm16_supported(16, 16, 96, 0, False, False, False)
    assert not mod.gemm16_supported(12, 16, 64, 0, True, False, False)
    assert not mod.gemm16_supported(16, 12, 64, 0, False, False, True)
    assert mod.gemm16_supported(16, 16, 64, 64, True, True, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ops_fall_back_to_the_library_for_refused_operands(dtype, monkeypatch):
    """linear16 / mm_kk / mm_nk16 with operands the kernel refuses return the
    right product through torch and never reach gemm16."""
    from pytorch_distributed_rnn_amd.ops import gemm as G

    class NoGemm16:
        def __init__(self, mod):
            self._mod = mod

        def __getattr__(self, name):
            if name == "gemm16":
                def refuse(*a, **k):
                    raise AssertionError("gemm16 reached with operands it refuses")
                return refuse
            return getattr(self._mod, name)

    native = G._native
    monkeypatch.setattr(G, "_native", lambda t: NoGemm16(native(t)) if native(t) is not None else None)
    g = R.gen(11)
    M, N = 40, 24

    def dev(x64, **kw):
        return R.in_nan(x64, dtype, 8, **kw)

    b64 = R.ints(N, g, lim=100)     # exact in 16 bits: the library path casts the bias to x's dtype
    for K, kw in ((100, {}), (64, dict(ld_extra=4)), (64, dict(shift=4))):    # K % 64; stride % 8; base alignment
        x, w = R.dyadic(M, K, g), R.dyadic(N, K, g)
        R.assert_within_ulp16(G.linear16(dev(x, **kw), dev(w), b64.float().cuda()), x @ w.t() + b64,
                              f"linear16 + bias {K} {kw}")
        R.assert_within_ulp16(G.linear16(dev(x, **kw), dev(w), None), x @ w.t(), f"linear16 {K} {kw}")
        wk = R.dyadic(K, N, g)
        R.assert_within_ulp16(G.mm_nk16([(dev(x, **kw), dev(wk))]), x @ wk, f"mm_nk16 {K} {kw}")
        a, b = R.dyadic(K, M, g), R.dyadic(K, N, g)
        R.assert_exact(G.mm_kk([(dev(a, **kw), dev(b))]), a.t() @ b, f"mm_kk {K} {kw}")
    # k-major M % 8 (mm_kk) / N % 8 (mm_nk16, 16-bit out), two pairs, accumulate_into
    a, b, a2, b2 = R.dyadic(64, 12, g), R.dyadic(64, N, g), R.dyadic(64, 12, g), R.dyadic(64, N, g)
    base = R.dyadic(12, N, g)
    acc = base.float().cuda()
    out = G.mm_kk([(dev(a), dev(b)), (dev(a2), dev(b2))], accumulate_into=acc)
    assert out.data_ptr() == acc.data_ptr()
    R.assert_exact(out, base + a.t() @ b + a2.t() @ b2, "mm_kk M % 8")
    x, wk, x2, wk2 = R.dyadic(M, 64, g), R.dyadic(64, 12, g), R.dyadic(M, 64, g), R.dyadic(64, 12, g)
    R.assert_within_ulp16(G.mm_nk16([(dev(x), dev(wk)), (dev(x2), dev(wk2))]), x @ wk + x2 @ wk2, "mm_nk16 N % 8",
                          rounded_first64=x @ wk)


# ---------------------------------------------------------------- derived bound, ordinary values
_RATIOS = {}


@pytest.mark.parametrize("mode", ["fp32", "split3", "out16"])
@pytest.mark.parametrize("akm,bkm", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm16_randn_within_derived_bound(dtype, akm, bkm, mode):
    """|C - ref| <= (K + S + 1) 2^-23 (|A| |B|) (+ u16 |ref|), 264 x 136 x 320.
    Worst error / bound over all layouts and dtypes on an MI355X: fp32 out
    0.0024, three splits 0.0013, 16-bit out 0.93 (bf16) / 0.77 (fp16) -- there
    the one output rounding is the whole error and the bound is its unit roundoff."""
    mod = _mod()
    M, N, K = 264, 136, 320
    torch.manual_seed(17)
    A64 = torch.randn(M, K).to(dtype).double()
    B64 = torch.randn(N, K).to(dtype).double()
    dA, dB = _store(A64, akm, dtype), _store(B64, bkm, dtype)
    S = 3 if mode == "split3" else 1
    C = mod.gemm16(dA, akm, dB, bkm, out16=(mode == "out16"), splitk=S)
    ratio = R.bound_ratio(C, A64, B64, S)
    _RATIOS[mode] = max(_RATIOS.get(mode, 0.0), ratio)
    print(f"gemm16 bound ratio {mode} {dtype} akm={akm} bkm={bkm}: {ratio:.4f} (worst so far {_RATIOS[mode]:.4f})")
    assert ratio <= 1.0
