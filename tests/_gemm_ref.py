"""Exact operands and padded buffers for the GEMM tests.

Dyadic operands.  :func:`dyadic` draws values ``m * 2**-3`` with integer
``|m| <= 16``.  Each is exact in bf16 (8 significant bits), fp16 and fp32.  A
product of two is a multiple of ``2**-6`` of magnitude at most 4, so any partial
sum of up to ``K_MAX = 16384`` products is a multiple of ``2**-6`` below
``2**24 * 2**-6``: it has at most 24 significant bits and is exact in fp32, in
whatever order the terms are added (``tests/test_gemm_ref_cpu.py`` shows this
on the CPU).  A correct kernel with fp32 accumulation therefore returns the
exact product, which an fp64 matmul on the CPU also computes exactly; a 16-bit
output is one round-to-nearest-even of it (:func:`round16`).  Integer biases
(:func:`ints`) and dyadic accumulate bases keep every sum inside that range
and push results onto bf16 / fp16 rounding ties.

Padding.  :func:`in_nan` stores an operand as an interior view of a NaN-filled
buffer (row stride > width, one NaN row above and below), :func:`Out` an output
as an interior view of a sentinel-filled buffer.  A read outside the operand
shows up as a NaN in the result, a write outside the output as a changed
sentinel.

The index arithmetic of the kernels that the tests assert case properties
with (tile raster, split-K ranges, fp32 GEMM tile selection) is mirrored here
in plain integers.
"""
import torch

MAG = 16          # |m| <= MAG
SCALE = 8         # values m / SCALE
K_MAX = 16384     # longest reduction the exactness argument covers
SENTINEL = -24576.0   # exact in bf16, fp16 and fp32; no dyadic result of the tests' shapes reaches it

U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def dyadic(rows, cols, g):
    """fp64 CPU [rows, cols] of values m / 8, |m| <= 16."""
    return torch.randint(-MAG, MAG + 1, (rows, cols), generator=g).double() / SCALE


def ints(n, g, lim=1000):
    """fp64 CPU [n] of integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, (n,), generator=g).double()


def round16(ref64, dtype):
    """The one round-to-nearest-even of an exact (fp32-representable) value."""
    return ref64.float().to(dtype)


def in_nan(x64, dtype, align, device="cuda", ld_extra=0, shift=0):
    """``x64`` in ``dtype`` as an interior view of a NaN-filled buffer: one NaN
    row above and below, ``align`` (+ ``shift``) NaN columns to the left, at
    least ``align`` to the right; row stride a multiple of ``align`` plus
    ``ld_extra``.  With shift = ld_extra = 0 the view's base is aligned to
    ``align`` elements (the buffer itself is allocator-aligned)."""
    rows, cols = x64.shape
    ld = -(-(cols + shift) // align) * align + 2 * align + ld_extra
    buf = torch.full((rows + 2, ld), float("nan"), dtype=dtype, device=device)
    v = buf[1:1 + rows, align + shift:align + shift + cols]
    v.copy_(x64.to(dtype))
    assert v.stride(0) == ld > cols and v.stride(1) == 1
    return v


class Out:
    """[M, N] output view inside a sentinel-filled buffer: two sentinel rows
    above and below and, with ``pad_cols``, ``align`` sentinel columns on both
    sides (row stride a multiple of ``align``); else contiguous."""

    def __init__(self, M, N, dtype, align=8, pad_cols=True, base64=None, device="cuda"):
        self.M, self.N = M, N
        self.off = align if pad_cols else 0
        ld = -(-N // align) * align + 2 * align if pad_cols else N
        self.buf = torch.full((M + 4, ld), SENTINEL, dtype=dtype, device=device)
        self.view = self.buf[2:2 + M, self.off:self.off + N]
        if base64 is not None:
            self.view.copy_(base64.to(dtype))
        assert pad_cols or self.view.is_contiguous()

    def assert_sentinels(self):
        chk = self.buf.clone()
        chk[2:2 + self.M, self.off:self.off + self.N] = SENTINEL
        bad = (chk != SENTINEL).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} sentinel(s) overwritten, first at buffer index {bad[0].tolist()} " \
                                 f"(output rows 2..{2 + self.M}, columns {self.off}..{self.off + self.N})"


def assert_exact(got, ref64, what=""):
    """``got`` (fp32 or 16-bit, any device) equals the exact fp64 value, cast
    to fp32 and then rounded once to got's dtype; no NaN.  Equal non-NaN values
    have equal bits (up to the sign of zero)."""
    g = got.detach().cpu()
    assert not torch.isnan(g).any(), f"{what}: NaN in the result (a read of the padding)"
    assert ref64.dtype == torch.float64 and g.shape == ref64.shape, (g.shape, ref64.shape)
    exp = ref64.float()
    assert torch.equal(exp.double(), ref64), f"{what}: reference not exact in fp32"
    if g.dtype != torch.float32:
        exp = exp.to(g.dtype)
    if not torch.equal(g, exp):
        bad = (g != exp).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ from the exact value; "
                             f"first at {i}: got {g[i].item()!r}, exact {exp[i].item()!r}")


def assert_within_ulp16(got, ref64, what="", rounded_first64=None):
    """A library-computed 16-bit result: within one unit roundoff of the exact
    value, ``|got - ref| <= u16 * |ref|`` (a single rounding gives u16 / 2).
    ``rounded_first64``: an exact intermediate the library rounds to 16 bits
    before adding the rest (a second product added with addmm_); its rounding
    error, at most ``u16 / 2`` of its magnitude, is allowed on top."""
    g = got.detach().cpu().double()
    assert not torch.isnan(g).any(), f"{what}: NaN"
    u = U16[got.dtype]
    err, bound = (g - ref64).abs(), u * ref64.abs()
    if rounded_first64 is not None:
        bound = bound + u * rounded_first64.abs()
    assert (err <= bound).all(), f"{what}: max excess {(err - bound).max().item():.3e}"


def bound_ratio(got, A64, B64, S, ref64=None):
    """max over the elements of |got - ref| / bound with the forward bound
    ``(K + S + 1) * 2**-23 * (|A| |B|)`` (+ ``u16 |ref|`` for a 16-bit result)
    of a sum of K + S terms in any order; A64 [M, K], B64 [N, K] fp64."""
    ref = A64 @ B64.t() if ref64 is None else ref64
    K = A64.shape[1]
    bound = (K + S + 1) * 2.0 ** -23 * (A64.abs() @ B64.abs().t())
    g = got.detach().cpu()
    if g.dtype != torch.float32:
        bound = bound + U16[g.dtype] * ref.abs()
    assert not torch.isnan(g).any()
    return ((g.double() - ref).abs() / bound).max().item()


# ---------------------------------------------------------------- kernel index arithmetic, mirrored
def gemm16_supported(M, N, K, K2, akm, bkm, out16, splitk=1, accumulate=False):
    """pdrnn_gemm_supported (csrc/kernels/gemm.hip)."""
    if M < 8 or N < 8 or K <= 0 or K % 64 or K2 % 64 or K2 < 0:
        return False
    if (akm and M % 8) or (bkm and N % 8):
        return False
    if out16 and (N % 8 or accumulate):
        return False
    if splitk > 1 and (out16 or (K + K2) // 64 < splitk):
        return False
    return True


def raster(tiles_m, tiles_n, group=4):
    """gemm_body's tile order: block id -> (tm, tn), with the group sizes used."""
    nwg = tiles_m * tiles_n
    q8, r8 = nwg >> 3, nwg & 7
    per_group = group * tiles_n
    out, sizes = [], set()
    for orig in range(nwg):
        xcd = orig & 7
        wg = (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3)
        first_m = (wg // per_group) * group
        gsz = min(tiles_m - first_m, group)
        sizes.add(gsz)
        out.append((first_m + (wg % per_group) % gsz, (wg % per_group) // gsz))
    return out, sizes


def split_ranges(KT1, KT2, S):
    """[(ktb, kte)] of the S splits over the KT1 + KT2 concatenated K-tiles."""
    KTALL = KT1 + KT2
    return [(KTALL * y // S, KTALL * (y + 1) // S) for y in range(S)]


def split_properties(KT1, KT2, S):
    """What a split-K case exercises in pp::mainloop and splitk_sum_kernel,
    from ktb = KTALL * y / S as the kernel computes it."""
    props = set()
    rng = split_ranges(KT1, KT2, S)
    assert all(e > b for b, e in rng), "a split without K-tiles"
    if all(e - b == 1 for b, e in rng):
        props.add("one_tile_per_split")
    if any(e - b == 1 for b, e in rng):
        props.add("one_tile_split")
    if any(e - b == 2 for b, e in rng):
        props.add("two_tile_split")
    for b, e in rng:
        if KT2 and b == KT1:
            props.add("starts_at_KT1")           # init() straight on segment 2
        if KT2 and b < KT1 < e:
            props.add(f"switch_at_t{KT1 - b}")   # issueA / issueB re-init at t = KT1 - ktb > 0
        if KT2 and e <= KT1:
            props.add("inside_segment1")
    props.add(f"sum8_rounds_{S // 8}_tail_{S % 8}")
    return props


def f32_plan(in_dtype, akm, M, N, K, K2=0):
    """gemm_f32's tile selection: (BN, BK, k-tiles)."""
    bn = 32 if N <= 32 else 64 if N <= 64 else 128
    bk = 32 if (in_dtype == torch.float32 and akm) else 16
    nt = -(-K // bk) + (-(-K2 // bk) if K2 > 0 else 0)
    return bn, bk, nt


def f32_vec(tensors):
    """The binding's ``vec`` flag: every row stride a multiple of 4 elements
    and every base aligned to 4 elements."""
    return all(t.stride(0) % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0 for t in tensors)


def f32_fast_tiles(vec, M, N, K, K2, bn, bk):
    """Number of workgroup tiles taking the unchecked (load_fast) loop, of all."""
    tiles_m, tiles_n = -(-M // 128), -(-N // bn)
    fast = 0
    for tm in range(tiles_m):
        for tn in range(tiles_n):
            if vec and tm * 128 + 128 <= M and tn * bn + bn <= N and K % bk == 0 and K2 % bk == 0:
                fast += 1
    return fast, tiles_m * tiles_n
