"""The weight-shadow pack kernel (csrc/kernels/shadow_pack.hip) job by job
against ``(src.float() + src2.float()).to(dtype)`` from the CPU, bit for bit
where finite and NaN where that is NaN: every source x destination dtype pair
(fp16 sources included), with and without ``src2``; extents around the 64 x 64
tile; the four read / write direction combinations of the tile path and a job
with no unit inner stride; the 4-wide vector path; batches that mix all of
them with zero-extent jobs; the special-value table of tests/_embedding_ref.py.
Sources are views inside NaN-filled buffers (a read outside shows as a NaN),
destinations views inside sentinel-filled buffers (a write outside changes a
sentinel).  And, at the model level, a replaced bias Parameter reaches the next
forward of a large-H LSTM (ops/shadow.py keys entries on the tensors
themselves).
"""
import itertools

import pytest
import torch

import _embedding_ref as E
from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.ops import shadow as sh

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
SENTINEL = -24576.0   # exact in all three dtypes
KINDS = ["unit2", "unit1", "strided"]   # which logical inner dimension has stride 1 in the buffer (none: "strided")
EXTENTS = [1, 63, 64, 65, 129]


def _view(buf_fill, n, kind, dtype, lead=3):
    """A logical [n0, n1, n2] view inside a filled buffer with one guard row
    around and ``lead`` guard elements before each row (3: no 4-element
    alignment, so never the vector path; 4: aligned)."""
    n0, n1, n2 = n
    if kind == "unit2":
        inner = -(-(n2 + lead) // 4) * 4 + 4
        buf = torch.full((n0, n1 + 2, inner), buf_fill, dtype=dtype, device=DEV)
        v = buf[:, 1:1 + n1, lead:lead + n2]
    elif kind == "unit1":
        inner = -(-(n1 + lead) // 4) * 4 + 4
        buf = torch.full((n0, n2 + 2, inner), buf_fill, dtype=dtype, device=DEV)
        v = buf[:, 1:1 + n2, lead:lead + n1].transpose(1, 2)
    else:
        buf = torch.full((n0, n1 + 2, 2 * n2 + 8), buf_fill, dtype=dtype, device=DEV)
        v = buf[:, 1:1 + n1, lead:lead + 2 * n2:2]
    assert tuple(v.shape) == tuple(n)
    return buf, v


class Job:
    def __init__(self, n, skind, dkind, sdt, ddt, with2, g, lead=3, values=None):
        self.n = n
        if values is None:
            a = torch.randn(n, generator=g) * 3
            b = torch.randn(n, generator=g)
        else:
            a, b = values
        _, self.src = _view(float("nan"), n, skind, sdt, lead)
        self.src.copy_(a.to(sdt))
        self.src2 = None
        if with2:
            _, self.src2 = _view(float("nan"), n, skind, sdt, lead)
            self.src2.copy_(b.to(sdt))
            assert self.src2.stride() == self.src.stride()
        self.dbuf, self.dst = _view(SENTINEL, n, dkind, ddt, lead)
        s = a.to(sdt).float()
        self.want = (s if not with2 else s + b.to(sdt).float()).to(ddt)

    def tup(self):
        return (self.dst, self.src, self.src2)

    def vec(self):
        """shadow_pack's vector-path condition (csrc/kernels/shadow_pack.hip)."""
        if self.dst.numel() == 0:
            return False   # no tile at all
        ok = self.src.stride(2) == 1 and self.dst.stride(2) == 1 and self.n[2] % 4 == 0
        ok = ok and all(t.stride(k) % 4 == 0 for t in (self.src, self.dst) for k in (0, 1))
        ptrs = [self.src] + ([self.src2] if self.src2 is not None else [])
        return ok and all(t.data_ptr() % (4 * t.element_size()) == 0 for t in ptrs + [self.dst])

    def check(self, what=""):
        E.assert_bits(self.dst, self.want, what)
        chk = self.dbuf.clone()
        # the view aliases dbuf: blank it out through the same indexing on the clone
        chk.as_strided(self.dst.shape, self.dst.stride(), self.dst.storage_offset()).fill_(SENTINEL)
        assert bool((chk == SENTINEL).all()), f"{what}: a sentinel around the destination was overwritten"


def _pack(jobs):
    n = _ext.require().shadow_pack([j.tup() for j in jobs])
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("with2", [False, True], ids=["src", "src+src2"])
@pytest.mark.parametrize("ddt", DTYPES, ids=IDS)
@pytest.mark.parametrize("sdt", DTYPES, ids=IDS)
def test_every_dtype_pair_on_every_path(sdt, ddt, with2):
    g = E.gen(DTYPES.index(sdt) * 3 + DTYPES.index(ddt))
    jobs = [Job((3, 65, 129), sk, dk, sdt, ddt, with2, g) for sk, dk in itertools.product(KINDS[:2], KINDS[:2])]
    jobs.append(Job((2, 63, 65), "strided", "strided", sdt, ddt, with2, g))
    jobs.append(Job((3, 5, 68), "unit2", "unit2", sdt, ddt, with2, g, lead=4))    # the vector path, n0 = 3
    assert [j.vec() for j in jobs] == [False] * 5 + [True]
    assert _pack(jobs) == 1
    for k, j in enumerate(jobs):
        j.check(f"job {k}")


@pytest.mark.parametrize("n0", [1, 3])
@pytest.mark.parametrize("skind,dkind", [("unit2", "unit2"), ("unit2", "unit1"), ("unit1", "unit2"), ("unit1", "unit1"),
                                         ("strided", "strided")])
def test_extents_around_the_tile(skind, dkind, n0):
    """n1, n2 in {1, 63, 64, 65, 129}: no, one and two partial tiles per
    dimension, in each direction combination (25 jobs, two launches)."""
    g = E.gen(n0 * 10 + KINDS.index(skind) * 3 + KINDS.index(dkind))
    jobs = [Job((n0, n1, n2), skind, dkind, torch.float32, torch.bfloat16, True, g) for n1 in EXTENTS for n2 in EXTENTS]
    assert not any(j.vec() for j in jobs)
    assert _pack(jobs) == 2
    for j in jobs:
        j.check(str(j.n))


def test_batch_mixing_vector_tile_and_zero_extent_jobs():
    g = E.gen(5)
    mk = lambda n, sk, dk, lead=3, ddt=torch.float16: Job(n, sk, dk, torch.float32, ddt, True, g, lead)
    jobs = [mk((0, 5, 8), "unit2", "unit2"),                   # zero extents first, between and last
            mk((3, 70, 132), "unit2", "unit2", lead=4),        # vector
            mk((2, 0, 8), "unit2", "unit1"),
            mk((1, 65, 66), "unit1", "unit2"),                 # tile, transposing
            mk((2, 64, 64), "unit2", "unit2", lead=4, ddt=torch.float32),   # vector, fp32 out
            mk((2, 7, 0), "unit1", "unit1"),
            mk((1, 129, 3), "unit2", "unit1"),
            mk((1, 1, 1), "strided", "strided"),
            mk((4, 3, 0), "unit2", "unit2")]
    assert [j.vec() for j in jobs] == [False, True, False, False, True, False, False, False, False]
    assert _pack(jobs) == 1
    for k, j in enumerate(jobs):
        j.check(f"job {k}")
    assert _pack([jobs[0], jobs[2]]) <= 1   # nothing to move: no fault, nothing written
    jobs[0].check(), jobs[2].check()


@pytest.mark.parametrize("ddt", DTYPES, ids=IDS)
@pytest.mark.parametrize("sdt", DTYPES, ids=IDS)
def test_special_values_on_both_paths(sdt, ddt):
    """Ties, range edges, fp16 subnormals, zeros, infinities, NaNs through the
    converting writers of the vector and the tile path; with ``src2`` the sums
    (inf - inf, overflow to inf) follow IEEE fp32 addition as on the CPU."""
    sv = E.special_values()
    sv = torch.cat([sv, torch.ones(-sv.numel() % 4)])   # the vector path takes multiples of 4
    n = (1, 2, sv.numel())
    a = torch.stack([sv, sv.flip(0)]).view(n)
    b = torch.stack([sv.flip(0), torch.zeros_like(sv)]).view(n)
    jobs = []
    for with2 in (False, True):
        jobs.append(Job(n, "unit2", "unit2", sdt, ddt, with2, None, lead=4, values=(a, b)))
        jobs.append(Job(n, "unit2", "unit1", sdt, ddt, with2, None, values=(a, b)))
    assert [j.vec() for j in jobs] == [True, False, True, False]
    assert _pack(jobs) == 1
    for k, j in enumerate(jobs):
        j.check(f"job {k}")


def test_replaced_bias_parameter_reaches_the_next_forward():
    """A large-H LSTM(64, 128) on bf16 input: after one forward a new
    ``bias_hh_l0`` Parameter is assigned (the old one stays referenced, as by
    an optimizer).  The next output is bit-equal to that of a freshly built
    module holding the same parameters."""
    from pytorch_distributed_rnn_amd.models.rnn import LSTM
    _ext.require()
    torch.manual_seed(11)
    m = LSTM(64, 128, 1).to(DEV)
    x = torch.randn(3, 4, 64, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        out0, _ = m(x)
    assert ("bias", 1, 128) in getattr(m.weight_ih_l0, "_pdrnn_shadow", {}), "not the large-H path"
    old = m.bias_hh_l0
    m.bias_hh_l0 = torch.nn.Parameter(old.detach() + 0.5)
    fresh = LSTM(64, 128, 1).to(DEV)
    fresh.load_state_dict(m.state_dict())
    before = sh.stats()["refreshes"]
    with torch.no_grad():
        out1, (h1, c1) = m(x)
        mid = sh.stats()["refreshes"]
        ref, (hr, cr) = fresh(x)
    torch.cuda.synchronize()
    assert mid == before + 1
    assert not torch.equal(out1, out0)
    assert torch.equal(out1, ref) and torch.equal(h1, hr) and torch.equal(c1, cr)
    assert old is not None
