"""Plain references and exact operands for the embedding and shadow-pack tests.

References.  :func:`gather` is ``w[idx]`` in fp64 after wrapping negative
indices; :func:`scatter_add` is the embedding's weight gradient, an fp64
``index_add_`` of the ``dout`` rows into ``[V, D]`` with the padding row zeroed
(plus an optional base, which the padding row keeps); :func:`stable_sort`
returns the permutation of a stable sort by wrapped row and the ``V + 1`` row
offsets.  ``tests/test_embedding_ref_cpu.py`` proves them against fp64
``F.embedding`` autograd and ``torch.sort(stable=True)``.

Exactness.  ``dout`` values are ``m / 8`` with integer ``|m| <= 16``
(``_gemm_ref.dyadic``): exact in bf16 (8 significant bits), fp16 and fp32.  A
sum of ``n`` of them is a multiple of ``2**-3`` of magnitude at most ``2 n``, so
it has at most 24 significant bits, and is exact in fp32 in whatever order the
terms are added, while ``16 n < 2**24``.  Every test built on this module has
``N <= 2**19`` contributions in all (``16 N <= 2**23``), so a correct kernel
that accumulates in fp32 returns exactly the fp64 sum and ``torch.equal`` is
the assertion.  Accumulate bases are dyadic too (``|m| <= 16``: one more
term).  The CPU test shows the order independence on fp32 sums.

Special values.  :func:`special_values` is an fp32 table of the values at
which a conversion to bf16 / fp16 goes wrong: rounding ties in both
directions and their neighbours, fp16's largest finite value and the tie above
it that rounds to infinity, the largest finite fp32, fp16-subnormal magnitudes
and ties among them, signed zeros, infinities and NaNs of several bit
patterns.  It holds no fp32 subnormal.  :func:`assert_bits` compares two
tensors bit for bit where the expectation is not NaN and with ``isnan`` where
it is (NaN payloads are not part of any contract here).
"""
import struct

import torch

from _gemm_ref import MAG, SCALE, gen  # noqa: F401  (re-exported for the tests)

N_MAX = 2 ** 19   # most contributions the exactness argument is used for


def wrap(idx, V):
    """Negative indices count from the last row."""
    return torch.where(idx < 0, idx + V, idx)


def gather(w64, idx):
    """``w64[idx]`` with negative indices wrapped: fp64 [*idx.shape, D]."""
    assert w64.dtype == torch.float64 and idx.dtype == torch.int64
    return w64[wrap(idx, w64.shape[0])]


def scatter_add(dout64, idx, V, padding_idx=None, base64=None):
    """The weight gradient: fp64 [V, D], row v the sum of the ``dout`` rows
    whose (wrapped) index is v, the padding row zero; added to ``base64``
    where given, whose padding row stays as it is."""
    assert dout64.dtype == torch.float64 and idx.dtype == torch.int64
    D = dout64.shape[-1]
    flat = wrap(idx.reshape(-1), V)
    assert flat.numel() == dout64.numel() // max(D, 1)
    out = torch.zeros(V, D, dtype=torch.float64, device=dout64.device)
    out.index_add_(0, flat, dout64.reshape(-1, D))
    if padding_idx is not None:
        out[padding_idx if padding_idx >= 0 else padding_idx + V] = 0
    return out if base64 is None else base64 + out


def stable_sort(idx, V):
    """(perm [N], offsets [V + 1]) of a stable sort of the wrapped indices:
    written as a counting sort in plain integers, independent of torch.sort."""
    flat = wrap(idx.reshape(-1), V)
    assert flat.numel() == 0 or (0 <= int(flat.min()) and int(flat.max()) < V)
    counts = torch.bincount(flat, minlength=V)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=idx.device)
    offsets[1:] = torch.cumsum(counts, 0)
    # position of element j: offsets[row] + number of earlier elements of the same row
    n = flat.numel()
    key = flat * max(n, 1) + torch.arange(n, device=idx.device)   # distinct keys, row-major then index order
    perm = torch.argsort(key)
    return perm, offsets


def dyadic_rows(shape, g, dtype=torch.float64):
    """fp64 (or ``dtype``) CPU tensor of values m / 8, |m| <= 16."""
    return (torch.randint(-MAG, MAG + 1, tuple(shape), generator=g).double() / SCALE).to(dtype)


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def special_bits():
    """int64 bit patterns of the fp32 special-value table."""
    pos = [
        0x3f808000, 0x3f818000,              # bf16 ties: to the even value below / above
        0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,   # and their neighbours
        0x3f801000, 0x3f803000,              # fp16 ties: down / up to even
        0x3f800fff, 0x3f801001, 0x3f802fff, 0x3f803001,
        0x477fe000,                          # 65504, fp16's largest finite
        0x477fefff, 0x477ff000, 0x477ff001,  # below, at (65520: rounds to inf) and above the tie to inf
        0x7f7fffff,                          # largest finite fp32: inf in both 16-bit types
        0x7f7f0000, 0x7f7f8000,              # bf16's largest finite; the tie above it
        0x33800000,                          # 2**-24: fp16's smallest subnormal
        0x33000000, 0x33000001, 0x32ffffff,  # 2**-25: tie to zero; just above (-> 2**-24); just below
        0x33c00000,                          # 3 * 2**-25: tie between 2**-24 and 2**-23 -> even
        0x38000000, 0x387fc000, 0x387fe000, 0x387ff000,   # 2**-15, largest fp16 subnormal, tie up to 2**-14
        0x38800000,                          # 2**-14: fp16's smallest normal
        0x3f800000, 0x40490fdb,              # 1, pi
        0x00800000,                          # smallest normal fp32
    ]
    bits = []
    for b in pos:
        bits += [b, b | 0x80000000]
    bits += [0x00000000, 0x80000000, 0x7f800000, 0xff800000]          # +-0, +-inf
    bits += [0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff, 0x7f800001, 0xff800001]   # NaNs
    return torch.tensor(bits, dtype=torch.int64)


def special_values():
    """The fp32 table (1-D CPU tensor), bit for bit from :func:`special_bits`."""
    b = special_bits()
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(torch.float32).clone()


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def assert_bits(got, want, what=""):
    """Bit-equal where ``want`` is not NaN; NaN exactly where ``want`` is."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    bad = (bits(got) != bits(want)) & ~nan
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits; first at {i}: "
                             f"got {got[i].item()!r} ({bits(got)[i].item() & (2 ** (8 * got.element_size()) - 1):#x}), "
                             f"want {want[i].item()!r} ({bits(want)[i].item() & (2 ** (8 * got.element_size()) - 1):#x})")


class Slab:
    """A contiguous [V, D] fp32 gradient inside a sentinel-filled 1-D buffer
    (``guard`` sentinels before and after), as a weight's slice of a flat
    gradient buffer is."""

    SENTINEL = -24576.0

    def __init__(self, V, D, base64=None, guard=64, device="cuda"):
        self.V, self.D, self.guard = V, D, guard
        self.buf = torch.full((V * D + 2 * guard,), self.SENTINEL, dtype=torch.float32, device=device)
        self.view = self.buf[guard:guard + V * D].view(V, D)
        self.view.copy_(base64.to(torch.float32) if base64 is not None else torch.zeros(V, D))
        assert self.view.is_contiguous()

    def assert_sentinels(self):
        g = self.guard
        assert bool((self.buf[:g] == self.SENTINEL).all()) and bool((self.buf[g + self.V * self.D:] == self.SENTINEL).all()), \
            "a sentinel next to the gradient slab was overwritten"


def in_nan_table(w64_or_f32, lead=0, device="cuda"):
    """An fp32 [V, D] table as a contiguous view inside a NaN-filled 1-D buffer,
    starting ``64 + lead`` floats into it (lead 0: 16-byte aligned)."""
    V, D = w64_or_f32.shape
    buf = torch.full((V * D + 128 + lead,), float("nan"), dtype=torch.float32, device=device)
    v = buf[64 + lead:64 + lead + V * D].view(V, D)
    v.copy_(w64_or_f32.to(torch.float32))
    assert v.is_contiguous() and (v.data_ptr() - buf.data_ptr()) == 4 * (64 + lead)
    return v
