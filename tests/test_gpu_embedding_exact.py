"""The embedding kernels (csrc/kernels/embedding.hip) and their host code
(bindings ``embedding_fwd`` / ``embedding_sort`` / ``embedding_bwd``,
``ops/embedding.py``) against the plain fp64 / int64 references of
tests/_embedding_ref.py, exactly.

The gather is a copy (fp32) or one round-to-nearest-even (bf16 / fp16), the
sort is integer work, and the backward runs on dyadic ``dout`` (multiples of
1/8, |x| <= 2) for which every fp32 partial sum is exact in any order (module
docstring of tests/_embedding_ref.py), so ``torch.equal`` with the fp64
reference is the assertion throughout.  The one exception, random-normal
``dout``, holds the derived bound ``|err| <= n_v * 2**-24 * sum_j |x_j|`` per
element (n_v: the row's contributions, one more term with a base).

Tables live in NaN-filled buffers (a row read outside the table shows as a
NaN), ``out=`` gradients in sentinel-guarded slabs.  The shapes are the
smallest that reach each path: the scalar and 16-byte gathers and their second
lane trip, the 16-bit gathers, the grid stride of every kernel (``blocks_for``
caps at 32768 waves), the CSR and the pieces backward with 2..32 pieces, the
thresholds between them, the sort's 256-index tile and 4096-index chunk.  No
test passes an out-of-range index.
"""
import time
from functools import lru_cache

import pytest
import torch

import _embedding_ref as E
from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.ops import gradsink
from pytorch_distributed_rnn_amd.ops.embedding import embedding

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]


def _mod():
    return _ext.require()


def _indices(V, N, g, shape=None):
    """Random rows in both spellings, the first and the last row in each."""
    idx = torch.randint(-V, V, (N,), generator=g)
    if N >= 4:
        idx[0], idx[1], idx[2], idx[3] = 0, V - 1, -1, -V
    return idx if shape is None else idx.view(shape)


# ------------------------------------------------------------------ forward, fp32
def _fwd_case(V, D, N, seed, lead=0):
    g = E.gen(seed)
    w64 = torch.randn(V, D, generator=g).double()   # fp32 values
    idx = _indices(V, N, g)
    w = E.in_nan_table(w64, lead)
    return w64, idx, w


@pytest.mark.parametrize("D", [1, 3, 5, 66, 130, 4, 68, 260, 1028])
def test_forward_fp32_scalar_and_vector_paths(D):
    """dim % 4 != 0: the scalar gather (second lane trip past 64 columns);
    dim % 4 == 0: 16 bytes a lane (second trip past 256)."""
    w64, idx, w = _fwd_case(37, D, 50, D)
    assert w.data_ptr() % 16 == 0
    out = _mod().embedding_fwd(w, idx.to(DEV))
    assert out.dtype == torch.float32 and out.shape == (50, D)
    assert torch.equal(out.cpu().double(), E.gather(w64, idx))


def test_forward_fp32_grid_stride():
    N = 40000   # > 32768 waves
    w64, idx, w = _fwd_case(37, 4, N, 7)
    out = _mod().embedding_fwd(w, idx.to(DEV))
    assert torch.equal(out.cpu().double(), E.gather(w64, idx))


@pytest.mark.parametrize("dtype", [None, torch.bfloat16, torch.float16], ids=DT_IDS)
def test_forward_transposed_indices_and_no_indices(dtype):
    w64, idx, w = _fwd_case(37, 68, 6 * 9, 11)
    idx_bt = idx.view(6, 9).to(DEV)
    idx_tb = idx_bt.t()
    assert not idx_tb.is_contiguous()
    out = _mod().embedding_fwd(w, idx_tb, dtype)
    want = E.gather(w64, idx.view(6, 9).t()).float()
    assert out.shape == (9, 6, 68)
    E.assert_bits(out, want if dtype is None else want.to(dtype))
    for shape in [(0,), (3, 0)]:
        empty = _mod().embedding_fwd(w, torch.empty(shape, dtype=torch.int64, device=DEV), dtype)
        torch.cuda.synchronize()
        assert empty.shape == (*shape, 68) and empty.dtype == (dtype or torch.float32)


@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("D", [4, 260])
def test_forward_fp32_weight_at_an_unaligned_storage_offset(D, lead):
    """A weight packed into a flat parameter buffer may start at any float:
    with dim % 4 == 0 the host then takes the scalar gather, not 16-byte
    loads from a base that is not 16-byte aligned."""
    w64, idx, w = _fwd_case(37, D, 50, 100 + D + lead, lead=lead)
    assert w.data_ptr() % 16 == 4 * lead and w.is_contiguous()
    out = _mod().embedding_fwd(w, idx.to(DEV))
    assert torch.equal(out.cpu().double(), E.gather(w64, idx))


# ------------------------------------------------------------------ forward, 16-bit
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [5, 64, 200])
def test_forward_16bit_is_one_rounding(dtype, D):
    g = E.gen(20 + D)
    V, N = 37, 300
    w32 = torch.randn(V, D, generator=g) * 4
    idx = _indices(V, N, g)
    out = _mod().embedding_fwd(E.in_nan_table(w32), idx.to(DEV), dtype)
    assert out.dtype == dtype and out.shape == (N, D)
    E.assert_bits(out, w32[E.wrap(idx, V)].to(dtype), f"{dtype} D={D}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, None], ids=["bf16", "fp16", "fp32"])
def test_forward_special_values(dtype):
    """Ties, the edges of the 16-bit ranges, fp16 subnormals, zeros,
    infinities, NaNs: the CPU's ``w[idx].to(dtype)``, bit for bit where finite
    (sign of zero included) and NaN where it is NaN."""
    sv = E.special_values()
    D = 70
    V = -(-sv.numel() // D) + 1
    w32 = sv.repeat(-(-V * D // sv.numel()))[:V * D].view(V, D).clone()
    idx = torch.cat([torch.arange(V), torch.arange(-V, 0)])
    out = _mod().embedding_fwd(E.in_nan_table(w32), idx.to(DEV), dtype)
    want = w32[E.wrap(idx, V)]
    E.assert_bits(out, want if dtype is None else want.to(dtype), str(dtype))


# ------------------------------------------------------------------ sort
def _check_sort(idx, V):
    perm, off = _mod().embedding_sort(idx.to(DEV), V)
    vals, ref_perm = torch.sort(E.wrap(idx, V), stable=True)
    assert perm.dtype == torch.int64 and off.dtype == torch.int64
    assert torch.equal(perm.cpu(), ref_perm)
    assert torch.equal(off.cpu(), torch.searchsorted(vals, torch.arange(V + 1)))
    p2, o2 = E.stable_sort(idx, V)
    assert torch.equal(perm.cpu(), p2) and torch.equal(off.cpu(), o2)


@pytest.mark.parametrize("V,N", [(1, 300), (5, 255), (5, 256), (5, 257), (300, 4096), (300, 4097), (300, 8191)])
def test_sort_at_tile_and_chunk_boundaries(V, N):
    _check_sort(torch.randint(-V, V, (N,), generator=E.gen(V * 10000 + N)), V)


def test_sort_all_equal_and_mixed_spellings():
    _check_sort(torch.full((8193,), 3), 5)
    _check_sort(torch.full((8193,), -2), 5)
    g = E.gen(31)
    rows = torch.randint(0, 5, (1000,), generator=g)
    neg = torch.randint(0, 2, (1000,), generator=g).bool()
    _check_sort(torch.where(neg, rows - 5, rows), 5)        # the same row as v and v - V, interleaved
    _check_sort(torch.tensor([2, -3] * 300), 5)


# ------------------------------------------------------------------ backward
CSR = [(300, 5, 1000), (300, 200, 5000), (7, 64, 0), (16384, 192, 20000)]
PIECES = [(1, 64, 64), (3, 70, 192 * 3), (4, 256, 4096), (100, 200, 30000)]
THRESHOLDS = [(3, 70, 192), (3, 70, 191)]     # N // V == 64: pieces; 63: CSR
MODES = ["returned", "out_base", "out_zeros"]


def takes_pieces(V, N):
    """embedding_bwd's path choice (csrc/bindings.cpp) and its piece count."""
    per_row = N // max(V, 1)
    if V <= 4096 and per_row >= 64:
        return min(32, max(2, per_row // 32))
    return 0


@lru_cache(maxsize=None)
def _bwd_case(V, D, N):
    """(idx, dout64, padding_idx, base64, ref64 without base) on the device;
    computed once and shared by every dtype and mode -- never modified."""
    g = E.gen(V * 1000003 + D * 1009 + N)
    pad = None
    if (V, D, N) == (4, 256, 4096):
        # row counts 4091, 5 (fewer than the 32 pieces), 0; row 3 is the padding row
        idx = torch.cat([torch.zeros(4091, dtype=torch.int64), torch.ones(5, dtype=torch.int64)])
        idx = idx[torch.randperm(N, generator=g)]
        idx = torch.where(torch.randint(0, 2, (N,), generator=g).bool(), idx - V, idx)
        pad = 3
    elif V == 1:
        idx = torch.randint(-1, 1, (N,), generator=g)
    else:
        idx = torch.randint(-V, V, (N,), generator=g)
        if N:
            pad = 1 if V < 8 else 5
            idx[: N // 5] = 2 if V < 8 else 3                     # a hot row
            if V >= 8:
                idx = torch.where((idx == 7) | (idx == 7 - V), idx + 1, idx)   # row 7 stays empty
            idx[-3:] = torch.tensor([pad, pad - V, pad])          # the padding row has contributions
    dout = E.dyadic_rows((N, D), g)
    base = E.dyadic_rows((V, D), g)
    idx, dout, base = idx.to(DEV), dout.to(DEV), base.to(DEV)
    ref = E.scatter_add(dout, idx, V, pad)
    assert N <= E.N_MAX and torch.equal(ref.float().double(), ref)
    if N and V > 1:
        counts = torch.bincount(E.wrap(idx, V), minlength=V)
        assert counts[pad] > 0 or (V, D, N) == (4, 256, 4096)
        assert (counts == 0).any() or V < 8
    return idx, dout, pad, base, ref


def _run_bwd(V, D, N, dt, mode):
    idx, dout, pad, base, ref = _bwd_case(V, D, N)
    g = dout.to(dt)
    assert torch.equal(g.double(), dout)
    padarg = -1 if pad is None else pad
    if mode == "returned":
        dw = _mod().embedding_bwd(g, idx, V, padarg)
        assert dw.dtype == torch.float32 and dw.shape == (V, D)
        assert torch.equal(dw.double(), ref), f"{int((dw.double() != ref).sum())} elements differ"
        if pad is not None:
            assert dw[pad].abs().max().item() == 0
        return
    b = base if mode == "out_base" else torch.zeros_like(base)
    slab = E.Slab(V, D, b)
    ret = _mod().embedding_bwd(g, idx, V, padarg, out=slab.view)
    assert ret.data_ptr() == slab.view.data_ptr()
    want = b + ref
    assert torch.equal(slab.view.double(), want), f"{int((slab.view.double() != want).sum())} elements differ"
    if pad is not None:
        assert torch.equal(slab.view[pad].double(), b[pad])     # the padding row keeps its base
    slab.assert_sentinels()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("V,D,N", CSR)
def test_backward_csr_path(V, D, N, dt, mode):
    """One wave per (row, 64 columns), the list walked 8 at a time; the last
    case has 16384 * 3 = 49152 waves and takes the grid stride."""
    assert takes_pieces(V, N) == 0
    _run_bwd(V, D, N, dt, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("V,D,N", PIECES)
def test_backward_pieces_path(V, D, N, dt, mode):
    assert takes_pieces(V, N) == {(1, 64, 64): 2, (3, 70, 576): 6, (4, 256, 4096): 32, (100, 200, 30000): 9}[(V, D, N)]
    _run_bwd(V, D, N, dt, mode)


@pytest.mark.parametrize("mode", ["returned", "out_base"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("V,D,N", THRESHOLDS)
def test_backward_either_side_of_the_rows_threshold(V, D, N, dt, mode):
    assert (takes_pieces(V, N) > 0) == (N == 192)
    _run_bwd(V, D, N, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_backward_either_side_of_the_vocabulary_threshold(dt):
    """The same indices (rows below 4096) and ``dout`` with V = 4096 (pieces)
    and V = 4097 (CSR): the same exact rows, the extra row zero."""
    N, D = 4097 * 64, 8
    assert takes_pieces(4096, N) == 2 and takes_pieces(4097, N) == 0
    g = E.gen(4096)
    idx = torch.randint(0, 4096, (N,), generator=g).to(DEV)
    dout = E.dyadic_rows((N, D), g).to(DEV)
    ref = E.scatter_add(dout, idx, 4096)
    a = _mod().embedding_bwd(dout.to(dt), idx, 4096, -1)
    b = _mod().embedding_bwd(dout.to(dt), idx, 4097, -1)
    assert torch.equal(a.double(), ref)
    assert torch.equal(b[:4096], a) and b[4096].abs().max().item() == 0


def test_backward_pieces_grid_stride():
    """512 rows x 9 slices x 8 pieces = 36864 waves > 32768: the pieces
    kernel's grid stride.  Generated and referenced on the device; prints its
    time (the one case here that is allowed more than a few seconds)."""
    V, D, N = 512, 576, 131072
    assert takes_pieces(V, N) == 8 and V * -(-D // 64) * 8 > 32768 and N <= E.N_MAX
    t0 = time.perf_counter()
    g = torch.Generator(device=DEV).manual_seed(5)
    idx = torch.randint(-V, V, (N,), generator=g, device=DEV)
    m = torch.randint(-E.MAG, E.MAG + 1, (N, D), generator=g, device=DEV, dtype=torch.int32)
    dout = (m.float() / E.SCALE).to(torch.bfloat16)
    del m
    ref = torch.zeros(V, D, dtype=torch.float64, device=DEV).index_add_(0, E.wrap(idx, V), dout.double())
    ref[9] = 0
    dw = _mod().embedding_bwd(dout, idx, V, 9)
    ok = torch.equal(dw.double(), ref)
    torch.cuda.synchronize()
    print(f"TIME pieces grid-stride case {time.perf_counter() - t0:.2f} s")
    assert ok and ref.abs().max().item() > 0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_backward_decodes_every_16bit_pattern(dt):
    """All 65536 patterns as ``dout``, one contribution per row: finite ones
    come back as their value, infinities keep their sign, NaNs stay NaN."""
    V = N = D = 256
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(N, D)
    dout = pat.view(dt)
    g = E.gen(77)
    rows = torch.randperm(V, generator=g)
    idx = torch.where(torch.randint(0, 2, (N,), generator=g).bool(), rows - V, rows)
    assert takes_pieces(V, N) == 0
    dw = _mod().embedding_bwd(dout.to(DEV), idx.to(DEV), V, -1).cpu()
    want = torch.zeros(V, D)
    want[rows] = dout.float()
    nan, inf = torch.isnan(want), torch.isinf(want)
    assert int(nan.sum()) > 0 and int(inf.sum()) == 2
    assert torch.equal(torch.isnan(dw), nan)
    assert torch.equal(dw[~nan], want[~nan])        # values, infinities with their sign
    fin = ~nan & ~inf
    assert torch.equal(dw[fin].double(), want[fin].double())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("V,D,N", [(300, 200, 5000), (100, 200, 30000)], ids=["csr", "pieces"])
def test_backward_random_normal_holds_the_summation_bound(V, D, N, dt):
    """Random-normal ``dout`` and base: ``|err| <= (n_v + 1) * 2**-24 *
    (sum_j |x_j| + |base|)`` per element against fp64 (each of the at most n_v
    inexact additions -- adding a zero or to a zero is exact -- is off by at
    most 2**-24 of a partial sum, itself at most the sum of magnitudes), the
    padding row equal to its base, and two runs bit-equal."""
    assert (takes_pieces(V, N) > 0) == (V == 100)
    g = E.gen(V + N)
    idx = torch.randint(-V, V, (N,), generator=g).to(DEV)
    idx[: N // 4] = 3
    pad = 5
    x = (torch.randn(N, D, generator=g) * 2).to(dt).to(DEV)
    base = torch.randn(V, D, generator=g).to(DEV)
    ref = E.scatter_add(x.double(), idx, V, pad, base.double())
    mag = E.scatter_add(x.double().abs(), idx, V, pad, base.double().abs())
    counts = torch.bincount(E.wrap(idx, V), minlength=V).double()
    counts[pad] = -1   # bound 0: the base itself
    bound = (counts + 1)[:, None] * 2.0 ** -24 * mag
    runs = []
    for _ in range(2):
        slab = E.Slab(V, D, base)
        _mod().embedding_bwd(x, idx, V, pad, out=slab.view)
        slab.assert_sentinels()
        runs.append(slab.view.clone())
    err = (runs[0].double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"RATIO embedding_bwd.random {worst:.4f}")
    assert (err <= bound).all(), f"worst error {worst:.3f} x the bound"
    assert torch.equal(runs[0][pad], base[pad])
    assert torch.equal(runs[0], runs[1])
    # returned (no base): n_v terms
    dw = _mod().embedding_bwd(x, idx, V, pad)
    ref0 = E.scatter_add(x.double(), idx, V, pad)
    bound0 = counts.clamp_min(0)[:, None] * 2.0 ** -24 * E.scatter_add(x.double().abs(), idx, V, pad)
    assert ((dw.double() - ref0).abs() <= bound0).all()
    assert torch.equal(dw, _mod().embedding_bwd(x, idx, V, pad))


# ------------------------------------------------------------------ ops.embedding.embedding
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "autograd"])
@pytest.mark.parametrize("pad", [None, 2, -1])
@pytest.mark.parametrize("V,D,T,B,odt", [(7, 6, 4, 3, None), (3, 70, 64, 3, torch.bfloat16)], ids=["csr", "pieces"])
def test_embedding_op_accumulates_into_a_preset_grad(V, D, T, B, odt, pad, direct):
    """A Parameter whose ``.grad`` already holds a dyadic base: with and
    without direct gradients ``.grad`` ends as base + reference exactly;
    ``padding_idx = -1`` is the last row, as in F.embedding, and the CPU
    fallback gives the same output and gradient."""
    g = E.gen(V + D + T)
    w32 = E.dyadic_rows((V, D), g, torch.float32)
    idx = torch.randint(0, V, (T, B), generator=g)    # F.embedding (the fallback) takes no negative index
    idx[0, 0], idx[0, 1] = 2, V - 1
    dout = E.dyadic_rows((T, B, D), g)
    base = E.dyadic_rows((V, D), g)
    ref = E.scatter_add(dout, idx, V, pad, base)
    if pad is not None:
        assert torch.equal(ref[pad], base[pad]) and E.scatter_add(dout, idx, V)[pad].abs().max() > 0
    got = {}
    for dev in (DEV, "cpu"):
        w = torch.nn.Parameter(w32.clone().to(dev))
        w.grad = base.float().to(dev)
        with gradsink.direct_grads(direct):
            out = embedding(idx.to(dev), w, out_dtype=odt, padding_idx=pad)
            out.backward(dout.to(out.dtype).to(dev))
        assert out.dtype == (odt or torch.float32)
        assert torch.equal(out.detach().cpu().double(), E.gather(w32.double(), idx))
        assert torch.equal(w.grad.cpu().double(), ref), dev
        got[dev] = (out.detach().cpu(), w.grad.cpu())
    assert torch.equal(got[DEV][0], got["cpu"][0]) and torch.equal(got[DEV][1], got["cpu"][1])


# ------------------------------------------------------------------ host checks
def test_host_checks_refuse_before_any_launch():
    mod = _mod()
    w = torch.zeros(5, 8, device=DEV)
    idx = torch.zeros(6, dtype=torch.int64, device=DEV)
    dout = torch.zeros(6, 8, device=DEV)
    with pytest.raises(RuntimeError, match="idx on"):
        mod.embedding_fwd(w, idx.cpu())
    with pytest.raises(RuntimeError, match="idx on"):
        mod.embedding_bwd(dout, idx.cpu(), 5, -1)
    with pytest.raises(RuntimeError, match="indices for"):
        mod.embedding_bwd(dout, idx[:5], 5, -1)
    with pytest.raises(RuntimeError, match="indices for"):
        mod.embedding_bwd(dout, torch.zeros(7, dtype=torch.int64, device=DEV), 5, -1)
    with pytest.raises(RuntimeError, match="out on"):
        mod.embedding_bwd(dout, idx, 5, -1, out=torch.zeros(5, 8))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        embedding(idx, torch.nn.Parameter(w), padding_idx=5)
