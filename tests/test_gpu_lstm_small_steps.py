"""lstm_small_fwd / lstm_small_bwd (csrc/kernels/lstm_small.hip) against the
fp64 reference of tests/_small_ref.py, per element, on every instantiation of
the fused small-H family that the bindings can launch.

Every case calls the bindings with explicit ``nb`` (sequences per workgroup)
and ``split`` (1: gate-split forward / unit-group backward, 2: K-split forward
/ row-split backward), so nothing here depends on what small_launch_config
chooses; the case's tag names the instantiation it runs:

    fwd  gs | ks   lstm | gru   H   train (SAVE) | infer   [stream (x not in LDS)]   nb 1 | 2
    bwd  unit | rowsplit   lstm | gru   H   [stream]   nb 1 | 2 | 3   [walk (grid < batch tiles)]

Bounds.  The forward of the training build is teacher-forced (_small_ref.py):
each step is evaluated in fp64 on the kernel's own stored hseq / act, so every
element of hseq, act, hn, cn must satisfy

    |kernel - ref| <= 2e-5 + 1e-4 |ref|                      (tests/test_gpu_lstm_large_steps.py)

The inference build stores nothing to force with: out / hn / cn are compared
with the free-running reference under the same bound, and so are dx, dh0 and
dc0 of the backward, which runs free in fp64 on the kernel's stored hseq / act
(the general kernels return no per-step gradients).  dparams are sums of B T
products; element (r, k) must lie within the budget the reference accumulates
next to the gradient,

    sum_{b,t} (2e-5 + 1e-4 |dg|) |in|  +  B T 2^-23 sum_{b,t} |dg| |in|       (biases: in = 1)

i.e. every product may carry the per-element bound of its gate gradient, and
an fp32 sum of n = B T terms in any order adds at most n ulps of the sum of
magnitudes.  grad_accum adds 2^-22 |prefill| for the rounding of the beta = 1
sum and of the subtraction that recovers the gradient.

The long streamed-x backward cases (T = 129 .. 385, weights halved so that the
recurrent Jacobian contracts) stay inside the same per-element bounds (worst
ratio below, rows "bwd ... stream"), so the fp32-run criterion is not used.

B = 5 leaves a half-empty last workgroup at nb = 2 and one empty slot at
nb = 3.  The persistent walk runs B = nb (cap + cap // 2) + 1, the smallest
batch of that form whose batch tiles exceed the resident cap for nb > 1 (for
nb = 1 it is cap + cap // 2 + 1).

The reference itself is proved against fp64 torch.nn.LSTM / nn.GRU autograd on
the CPU, and the comparison is shown to reject six planted defects
(test_reference_matches_torch_fp64, test_comparison_rejects_defect; not gpu).

Worst |kernel - ref| / bound per instantiation and tensor, measured on an
MI355X when this file was written:

    bwd rowsplit lstm H16 nb1          dparams 0.000  dx 0.001  dh0 0.000  dc0 0.000
    bwd rowsplit lstm H32 nb1          dparams 0.005  dx 0.001  dh0 0.000  dc0 0.001
    bwd rowsplit lstm H32 stream nb1   dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd rowsplit lstm H64 nb1          dparams 0.000  dx 0.001  dh0 0.000  dc0 0.000
    bwd unit gru H16 nb1               dparams 0.000  dx 0.001  dh0 0.001
    bwd unit gru H32 nb1               dparams 0.002  dx 0.000  dh0 0.000
    bwd unit gru H64 nb1               dparams 0.000  dx 0.001  dh0 0.000
    bwd unit lstm H16 nb1              dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H16 nb2              dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H16 nb3              dparams 0.003  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H32 nb1              dparams 0.004  dx 0.001  dh0 0.000  dc0 0.000
    bwd unit lstm H32 nb1 walk         dparams 0.000  dx 0.001  dh0 0.000  dc0 0.001
    bwd unit lstm H32 nb2              dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H32 nb3              dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H32 nb3 walk         dparams 0.000  dx 0.001  dh0 0.000  dc0 0.001
    bwd unit lstm H32 stream nb1       dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H32 stream nb2       dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H32 stream nb3       dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H64 nb1              dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    bwd unit lstm H64 stream nb1       dparams 0.000  dx 0.000  dh0 0.000  dc0 0.000
    fwd gs gru H16 infer nb1           hn 0.004  out 0.005
    fwd gs gru H16 infer nb2           hn 0.005  out 0.004
    fwd gs gru H16 infer stream nb2    hn 0.003  out 0.005
    fwd gs gru H16 train nb1           hseq 0.003  act 0.006  hn 0.003
    fwd gs gru H16 train nb2           hseq 0.005  act 0.007  hn 0.005
    fwd gs gru H16 train stream nb2    hseq 0.003  act 0.006  hn 0.002
    fwd gs gru H32 infer nb1           hn 0.003  out 0.004
    fwd gs gru H32 infer nb2           hn 0.004  out 0.005
    fwd gs gru H32 infer stream nb1    hn 0.003  out 0.004
    fwd gs gru H32 train nb1           hseq 0.004  act 0.007  hn 0.003
    fwd gs gru H32 train nb2           hseq 0.003  act 0.006  hn 0.003
    fwd gs gru H32 train stream nb1    hseq 0.004  act 0.006  hn 0.003
    fwd gs gru H64 infer nb1           hn 0.004  out 0.004
    fwd gs gru H64 infer nb2           hn 0.003  out 0.004
    fwd gs gru H64 train nb1           hseq 0.003  act 0.006  hn 0.003
    fwd gs gru H64 train nb2           hseq 0.004  act 0.007  hn 0.003
    fwd gs lstm H16 infer nb1          hn 0.004  out 0.004  cn 0.004
    fwd gs lstm H16 infer nb2          hn 0.004  out 0.004  cn 0.004
    fwd gs lstm H16 infer stream nb2   hn 0.003  out 0.006  cn 0.004
    fwd gs lstm H16 train nb1          hseq 0.004  act 0.006  hn 0.004  cn 0.004
    fwd gs lstm H16 train nb2          hseq 0.004  act 0.006  hn 0.003  cn 0.002
    fwd gs lstm H16 train stream nb2   hseq 0.005  act 0.007  hn 0.003  cn 0.003
    fwd gs lstm H32 infer nb1          hn 0.004  out 0.005  cn 0.005
    fwd gs lstm H32 infer nb2          hn 0.004  out 0.005  cn 0.005
    fwd gs lstm H32 infer stream nb1   hn 0.004  out 0.005  cn 0.003
    fwd gs lstm H32 infer stream nb2   hn 0.003  out 0.005  cn 0.003
    fwd gs lstm H32 train nb1          hseq 0.004  act 0.006  hn 0.003  cn 0.003
    fwd gs lstm H32 train nb2          hseq 0.005  act 0.007  hn 0.004  cn 0.003
    fwd gs lstm H32 train stream nb1   hseq 0.005  act 0.006  hn 0.003  cn 0.003
    fwd gs lstm H32 train stream nb2   hseq 0.004  act 0.006  hn 0.003  cn 0.002
    fwd gs lstm H64 infer nb1          hn 0.004  out 0.004  cn 0.004
    fwd gs lstm H64 infer nb2          hn 0.003  out 0.003  cn 0.004
    fwd gs lstm H64 infer stream nb1   hn 0.003  out 0.004  cn 0.003
    fwd gs lstm H64 train nb1          hseq 0.004  act 0.007  hn 0.004  cn 0.003
    fwd gs lstm H64 train nb2          hseq 0.004  act 0.005  hn 0.004  cn 0.003
    fwd gs lstm H64 train stream nb1   hseq 0.004  act 0.007  hn 0.003  cn 0.002
    fwd ks lstm H32 infer nb1          hn 0.003  out 0.002  cn 0.004
    fwd ks lstm H32 infer nb2          hn 0.002  out 0.002  cn 0.004
    fwd ks lstm H32 infer stream nb1   hn 0.001  out 0.003  cn 0.003
    fwd ks lstm H32 infer stream nb2   hn 0.002  out 0.003  cn 0.003
    fwd ks lstm H32 train nb1          hseq 0.004  act 0.006  hn 0.004  cn 0.004
    fwd ks lstm H32 train nb2          hseq 0.002  act 0.006  hn 0.002  cn 0.003
    fwd ks lstm H32 train stream nb1   hseq 0.005  act 0.007  hn 0.004  cn 0.002
    fwd ks lstm H32 train stream nb2   hseq 0.002  act 0.006  hn 0.001  cn 0.003
    fwd ks lstm H64 infer nb1          hn 0.002  out 0.003  cn 0.004
    fwd ks lstm H64 infer nb2          hn 0.002  out 0.002  cn 0.005
    fwd ks lstm H64 infer stream nb1   hn 0.002  out 0.002  cn 0.003
    fwd ks lstm H64 train nb1          hseq 0.004  act 0.006  hn 0.003  cn 0.003
    fwd ks lstm H64 train nb2          hseq 0.002  act 0.007  hn 0.002  cn 0.002
    fwd ks lstm H64 train stream nb1   hseq 0.004  act 0.006  hn 0.004  cn 0.003

The 264 GPU cases take 4.3 s together.
"""
import collections
import copy
import math

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.ops import gru_fused
from pytorch_distributed_rnn_amd.ops import lstm as lstm_ops

import _small_ref as R
from _tune import set_tune

gpu = pytest.mark.gpu
F64 = torch.float64

_worst = collections.defaultdict(float)  # (instantiation, tensor) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nworst |kernel - ref| / bound per instantiation and tensor")
        rows = collections.defaultdict(dict)
        for (tag, name), v in _worst.items():
            rows[tag][name] = v
        for tag in sorted(rows):
            print(f"RATIO {tag:34s} " + "  ".join(f"{n} {v:.3f}" for n, v in rows[tag].items()))


def compare(tag, got, ref, budget=None, extra=None, worst=None):
    """Every tensor of ``got`` against ``ref`` per element; dparams against the
    reference's budget (+ ``extra``).  Records the worst ratio per (tag, tensor)
    and raises naming every tensor that misses."""
    bad = []
    for name, a in got.items():
        b = ref[name]
        assert a.shape == b.shape, (tag, name, tuple(a.shape), tuple(b.shape))
        bound = budget if name == "dparams" else R.ATOL + R.RTOL * b.abs()
        if extra is not None and name == "dparams":
            bound = bound + extra
        diff = (a.double() - b).abs()
        if not bool(torch.isfinite(a).all()):
            ratio = float("inf")
        else:
            exact = torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf")))
            q = torch.where(bound > 0, diff / bound.clamp_min(1e-300), exact)
            ratio = float(q.max()) if q.numel() else 0.0
        if worst is not None:
            worst[(tag, name)] = max(worst[(tag, name)], ratio)
        if not ratio <= 1.0:
            bad.append((name, round(ratio, 3)))
    assert not bad, (tag, bad)


# ---------------------------------------------------------------------------
# the reference against torch, fp64, CPU
# ---------------------------------------------------------------------------
def _module_weights(m, NL, bias):
    ws = []
    for l in range(NL):
        ws += [getattr(m, f"weight_ih_l{l}"), getattr(m, f"weight_hh_l{l}")]
        ws += [getattr(m, f"bias_ih_l{l}"), getattr(m, f"bias_hh_l{l}")] if bias else [None, None]
    return ws


@pytest.mark.parametrize("loss", ["out", "final", "both"])
@pytest.mark.parametrize("bias,state", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("NL", [1, 2, 3])
@pytest.mark.parametrize("cell", [0, 1])
def test_reference_matches_torch_fp64(cell, NL, bias, state, loss):
    """Free-running, the reference equals fp64 nn.LSTM / nn.GRU to 1e-10:
    outputs, final states, every parameter gradient in the flat order, dx,
    dh0, dc0.  The GRU goes through the production packing (gru_fused._pack)
    and its gradients back through gru_fused._unpack_index."""
    torch.manual_seed(100 * cell + 10 * NL + 2 * bias + state)
    H, B, T, I = 5, 3, 4, 3
    lstm = cell == 0
    m = (torch.nn.LSTM if lstm else torch.nn.GRU)(I, H, NL, bias=bias, batch_first=True).double()
    x = torch.randn(B, T, I, dtype=F64, requires_grad=True)
    h0 = torch.randn(NL, B, H, dtype=F64, requires_grad=True) if state else None
    c0 = torch.randn(NL, B, H, dtype=F64, requires_grad=True) if state and lstm else None
    if lstm:
        out, (hn, cn) = m(x, (h0, c0) if state else None)
    else:
        out, hn = m(x, h0)
        cn = None
    g = torch.randn_like(out) if loss != "final" else None
    ghn = torch.randn_like(hn) if loss != "out" else None
    gcn = torch.randn_like(cn) if lstm and loss != "out" else None
    sum((a * b).sum() for a, b in ((out, g), (hn, ghn), (cn, gcn)) if b is not None).backward()

    tol = dict(rtol=0, atol=1e-10)
    with torch.no_grad():
        ws = _module_weights(m, NL, bias)
        w = ws if lstm else gru_fused._pack(ws, NL, H, x.detach())
        h0d, c0d = (h0.detach() if state else None), (c0.detach() if c0 is not None else None)
        hseq, act, rhn, rcn = R.forward(x, w, h0d, c0d, H, NL, cell)
        for a, b in zip(R.forward(x, w, h0d, c0d, H, NL, cell, forced=(hseq, act)), (hseq, act, rhn, rcn)):
            torch.testing.assert_close(a, b, rtol=0, atol=1e-13)  # forcing with its own results changes nothing
        torch.testing.assert_close(hseq[NL - 1], out, **tol)
        torch.testing.assert_close(rhn, hn, **tol)
        if lstm:
            torch.testing.assert_close(rcn, cn, **tol)
        dparams, budget, dx, dh0, dc0 = R.backward(x, w, h0d, c0d, hseq, act, g, ghn, gcn, H, NL, cell)
        assert dparams.shape == budget.shape and bool((budget > 0).all())
        if lstm:
            want = torch.cat([p.grad.reshape(-1) for p in ws if p is not None])
            assert R.flat_offsets(w, NL)[-1][0] == want.numel()
        else:  # packed gradients always carry the bias blocks; nn.GRU's order after the unpack
            in_dims = tuple(int(w[4 * l].shape[1]) for l in range(NL))
            dparams = dparams.index_select(0, gru_fused._unpack_index(H, in_dims, dparams.device))
            parts, off = [], 0
            for l, Il in enumerate(in_dims):
                for k, n in enumerate((3 * H * Il, 3 * H * H, 3 * H, 3 * H)):
                    if ws[4 * l + k] is not None:
                        parts.append(dparams[off:off + n])
                    off += n
            dparams = torch.cat(parts)
            want = torch.cat([p.grad.reshape(-1) for p in ws if p is not None])
        torch.testing.assert_close(dparams, want, **tol)
        torch.testing.assert_close(dx, x.grad, **tol)
        if state:
            torch.testing.assert_close(dh0, h0.grad, **tol)
            if lstm:
                torch.testing.assert_close(dc0, c0.grad, **tol)


# ---------------------------------------------------------------------------
# the comparison rejects planted defects (CPU)
# ---------------------------------------------------------------------------
def _defect_case():
    torch.manual_seed(5)
    H, NL, B, T, I = 8, 2, 5, 7, 3
    k = 1.0 / math.sqrt(H)
    w = []
    for l in range(NL):
        Il = I if l == 0 else H
        w += [(torch.rand(4 * H, Il, dtype=F64) * 2 - 1) * k, (torch.rand(4 * H, H, dtype=F64) * 2 - 1) * k,
              (torch.rand(4 * H, dtype=F64) * 2 - 1) * k, (torch.rand(4 * H, dtype=F64) * 2 - 1) * k]
    x = torch.randn(B, T, I, dtype=F64) * 0.5
    h0, c0 = torch.randn(NL, B, H, dtype=F64) * 0.5, torch.randn(NL, B, H, dtype=F64) * 0.5
    dout, dhn, dcn = (torch.randn(B, T, H, dtype=F64) * 0.1, torch.randn(NL, B, H, dtype=F64) * 0.1,
                      torch.randn(NL, B, H, dtype=F64) * 0.1)
    hseq, act, hn, cn = R.forward(x, w, h0, c0, H, NL)
    dparams, budget, dx, dh0, dc0 = R.backward(x, w, h0, c0, hseq, act, dout, dhn, dcn, H, NL)
    ref = dict(hseq=hseq, act=act, hn=hn, cn=cn, dparams=dparams, dx=dx, dh0=dh0, dc0=dc0)
    args = dict(x=x, w=w, h0=h0, c0=c0, dout=dout, dhn=dhn, dcn=dcn, H=H, NL=NL, B=B)
    return ref, budget, args


def _fp32(ref):
    return {k: v.float() for k, v in ref.items()}


def _defect(kind, ref, a):
    """The fp64 reference rounded to fp32, with one defect."""
    got = _fp32(ref)
    H, NL, B = a["H"], a["NL"], a["B"]
    hseq, act = ref["hseq"], ref["act"]

    def bwd(**over):
        k = dict(a, **over)
        return R.backward(k["x"], k["w"], k["h0"], k["c0"], over.get("hseq", hseq), over.get("act", act), k["dout"],
                          k["dhn"], k["dcn"], H, NL)
    if kind == "f and o slots swapped in one layer":
        got["act"][1] = got["act"][1][:, :, [0, 3, 2, 1, 4]]
    elif kind == "dcn term dropped":
        dp, _, dx, dh0, dc0 = bwd(dcn=None)
        got.update(dparams=dp.float(), dx=dx.float(), dh0=dh0.float(), dc0=dc0.float())
    elif kind == "h0 contribution to dW_hh at t = 0 dropped":
        got["dparams"] = bwd(h0=None)[0].float()  # h0 enters the LSTM's backward through dW_hh alone
        changed = (got["dparams"] != ref["dparams"].float()).nonzero().flatten()
        offs = R.flat_offsets(a["w"], NL)
        assert all(any(o[1] <= int(i) < o[2] for o in offs[:NL]) for i in changed) and changed.numel() > 0
    elif kind == "last batch row left out of dparams":
        dg = R.gate_grads(a["w"], a["h0"], a["c0"], hseq, act, a["dout"], a["dhn"], a["dcn"], H, NL)[0]
        got["dparams"] = R.param_grads(dg, a["x"], a["h0"], hseq, True, rows=slice(0, B - 1))[0].float()
    elif kind == "db_hh zero while db_ih is right":
        o = R.flat_offsets(a["w"], NL)[0]
        got["dparams"][o[3]:o[3] + 4 * H] = 0
    elif kind == "one dx column shifted by one":
        got["dx"][:, 1:, 0] = ref["dx"][:, :-1, 0].float()  # column 0 arrives one step late
    else:
        raise KeyError(kind)
    return got


_DEFECTS = ["f and o slots swapped in one layer", "dcn term dropped", "h0 contribution to dW_hh at t = 0 dropped",
            "last batch row left out of dparams", "db_hh zero while db_ih is right", "one dx column shifted by one"]


def test_comparison_accepts_rounded_reference():
    ref, budget, _ = _defect_case()
    compare("cpu", _fp32(ref), ref, budget)


@pytest.mark.parametrize("kind", _DEFECTS)
def test_comparison_rejects_defect(kind):
    """One wrong slot order, dropped term, dropped row, zeroed bias slot or
    shifted column (column 0 of dx one step late) fails the comparison that
    the undamaged fp32 copy passes."""
    ref, budget, args = _defect_case()
    got = _defect(kind, ref, args)
    with pytest.raises(AssertionError) as e:
        compare("cpu", got, ref, budget)
    named = {"f and o": "act", "dcn": "dc0", "h0 contribution": "dparams", "last batch": "dparams", "db_hh": "dparams",
             "one dx": "dx"}
    assert [v for k, v in named.items() if kind.startswith(k)][0] in str(e.value)


# ---------------------------------------------------------------------------
# the kernels against the reference
# ---------------------------------------------------------------------------
_XLDS_BYTES = 48 * 1024
CELLS = {0: "lstm", 1: "gru"}

# input variants of the forward, spread over its matrix (see _fwd_matrix)
_FWD_VARIANTS = [
    dict(I=9, state=True, bias=True, batch_first=True, x="plain"),
    dict(I=1, state=False, bias=False, batch_first=False, x="plain"),
    dict(I="H", state=True, bias=True, batch_first=True, x="wide"),
    dict(I=9, state=False, bias=True, batch_first=True, x="idx"),
    dict(I=9, state=True, bias=False, batch_first=True, x="bf16"),
    dict(I="H", state=True, bias=True, batch_first=False, x="plain"),
    dict(I=1, state=True, bias=True, batch_first=False, x="wide"),
    dict(I="H", state=False, bias=False, batch_first=True, x="idx"),
]
# what a backward case passes: "full" everything; "bare" dout alone, zero state,
# parameter gradients only; "final" no dout; "strided" dout a column slice of a
# wider tensor, seq-first; "idx" gathered x (no dx); "bf16" bf16 x; "nobias"
_BWD_VARIANTS = {
    "full": dict(I=9),
    "bare": dict(I=9, state=False, final=False, need_dx=False, need_dh0=False),
    "final": dict(I=1, seq=False),
    "strided": dict(I="H", batch_first=False, strided=True),
    "idx": dict(I=9, x="idx", need_dx=False),
    "bf16": dict(I=9, x="bf16"),
    "nobias": dict(I="H", bias=False),
}


def _xlds(H, nb, T):
    return nb * T * H * 4 <= _XLDS_BYTES


def _fwd_tag(split, cell, save, H, nb, T):
    return (f"fwd {'gs' if split == 1 else 'ks'} {CELLS[cell]} H{H} {'train' if save else 'infer'}"
            f"{'' if _xlds(H, nb, T) else ' stream'} nb{nb}")


def _bwd_tag(split, cell, H, nb, T, walk=False):
    return (f"bwd {'unit' if split == 1 else 'rowsplit'} {CELLS[cell]} H{H}{'' if _xlds(H, nb, T) else ' stream'} nb{nb}"
            f"{' walk' if walk else ''}")


class _Inputs:
    pass


def _inputs(H, NL, cell, B, T, I, seed, *, state=True, bias=True, batch_first=True, x="plain", wscale=1.0):
    """Operands of one case.  ``x``: plain | wide (the middle I columns of a
    NaN-filled tensor) | idx (gathered from a larger table, rows repeated) |
    bf16.  s.x_ref is the batch-major fp32 image the reference runs on."""
    dev = "cuda"
    torch.manual_seed(seed)
    s = _Inputs()
    I = H if I == "H" else I
    k = wscale / math.sqrt(H)
    G = 4 if cell == 0 else 3
    ws = []
    for l in range(NL):
        Il = I if l == 0 else H
        ws += [(torch.rand(G * H, Il) * 2 - 1) * k, (torch.rand(G * H, H) * 2 - 1) * k]
        ws += [(torch.rand(G * H) * 2 - 1) * k, (torch.rand(G * H) * 2 - 1) * k] if bias else [None, None]
    ws = [t.to(dev) if t is not None else None for t in ws]
    if cell == 1:
        packed = gru_fused._pack(ws, NL, H, torch.empty(0, device=dev))
        ws = [t if (bias or j % 4 < 2) else None for j, t in enumerate(packed)]
    s.w = ws
    s.h0 = (torch.randn(NL, B, H) * 0.5).to(dev) if state else None
    s.c0 = (torch.randn(NL, B, H) * 0.5).to(dev) if state and cell == 0 else None
    s.idx = None
    s.batch_first = batch_first
    if x == "idx":
        assert batch_first
        table = (torch.randn(B + 3, T, I) * 0.5).to(dev)
        s.idx = (torch.arange(B) * 5 % (B + 3)).to(dev)
        s.idx[B - 1] = s.idx[0]  # a repeated row
        s.x, s.x_ref = table, table[s.idx]
    else:
        base = torch.randn(B, T, I) * 0.5
        if x == "bf16":
            base = base.to(torch.bfloat16)
        base = base.to(dev)
        lay = base if batch_first else base.transpose(0, 1).contiguous()
        if x == "wide":
            wide = torch.full(lay.shape[:2] + (I + 9,), float("nan"), device=dev)
            wide[..., 5:5 + I] = lay
            lay = wide[..., 5:5 + I]
            assert lay.stride(1) > I and lay.stride(2) == 1
        s.x, s.x_ref = lay, base.float()
    return s


def _bm(t, batch_first):
    """[B, T, *] view of a kernel tensor laid out as x is."""
    return t if batch_first else t.transpose(0, 1)


def _forward_case(H, NL, cell, nb, split, save, T, B, variant, seed, wscale=1.0):
    mod = _ext.require()
    v = dict(variant)
    need_out = v.pop("need_out", True)
    s = _inputs(H, NL, cell, B, T, v.pop("I"), seed, wscale=wscale, **v)
    if cell == 1:
        assert lstm_ops.small_plan(s.x_ref, H, NL, cell="gru") == (H, [(0, NL)])  # one unpadded launch
    out, hn, cn, act = mod.lstm_small_fwd(s.x, s.idx, s.w, s.h0, s.c0, H, NL, s.batch_first, save, need_out, nb,
                                          split, cell)
    torch.cuda.synchronize()
    tag = _fwd_tag(split, cell, save, H, nb, T)
    if save:
        assert out.shape == (NL, B, T, H) and act.shape == (NL, B, T, 5, H)
        rh, ra, rhn, rcn = R.forward(s.x_ref, s.w, s.h0, s.c0, H, NL, cell, forced=(out, act))
        got, ref = dict(hseq=out, act=act, hn=hn), dict(hseq=rh, act=ra, hn=rhn)
    else:
        assert act is None
        rh, _, rhn, rcn = R.forward(s.x_ref, s.w, s.h0, s.c0, H, NL, cell)
        got, ref = dict(hn=hn), dict(hn=rhn)
        if need_out:
            assert out.shape == ((B, T, H) if s.batch_first else (T, B, H)) and out.is_contiguous()
            got["out"], ref["out"] = _bm(out, s.batch_first), rh[NL - 1]
        else:
            assert out is None
    if cell == 0:  # the GRU's cn is left unwritten
        got["cn"], ref["cn"] = cn, rcn
    compare(tag, got, ref, worst=_worst)
    return s, out, act


def _fwd_matrix():
    rows, k = [], 0
    shapes = [(16, 1), (16, 4), (32, 2), (32, 4), (64, 1)]
    for split, cell, hs in ((1, 0, shapes), (1, 1, shapes), (2, 0, shapes[2:] + [(32, 1)])):
        for H, NL in hs:
            # shape k of the 14: variant k for nb 1, k + 4 for nb 2, the
            # inference build three places ahead -- every (build, nb) walks
            # all eight variants over the matrix
            for nb in (1, 2):
                for save in (True, False):
                    var = (k + 4 * (nb - 1) + (0 if save else 3)) % len(_FWD_VARIANTS)
                    rows.append(pytest.param(split, cell, H, NL, nb, save, var,
                                             id=f"{'gs' if split == 1 else 'ks'}-{CELLS[cell]}-H{H}x{NL}-nb{nb}-"
                                                f"{'train' if save else 'infer'}-v{var}"))
            k += 1
    return rows


@gpu
@pytest.mark.parametrize("split,cell,H,NL,nb,save,var", _fwd_matrix())
def test_forward(split, cell, H, NL, nb, save, var):
    """Gate-split (LSTM, GRU) and K-split (LSTM) forward, training and
    inference builds, 1 and 2 sequences per workgroup; T = 7 fills and drains
    the layer pipeline, B = 5 leaves the last workgroup of nb = 2 half empty."""
    variant = dict(_FWD_VARIANTS[var])
    if cell == 1 and variant["x"] == "bf16":
        variant["x"] = "plain"  # gru_fused admits fp32 x only
    _forward_case(H, NL, cell, nb, split, save, 7, 5, variant, seed=1000 * split + 100 * cell + H + NL + nb)


@gpu
@pytest.mark.parametrize("split,cell,H,NL,nb", [(1, 0, 32, 2, 1), (1, 0, 16, 4, 2), (1, 1, 64, 1, 1), (1, 1, 32, 4, 2),
                                                (2, 0, 32, 4, 1), (2, 0, 64, 1, 2)])
def test_forward_without_out(split, cell, H, NL, nb):
    """need_out = False: the inference build returns no output stream and the
    final states are unchanged."""
    variant = dict(_FWD_VARIANTS[(H + nb) % len(_FWD_VARIANTS)], need_out=False)
    if cell == 1 and variant["x"] == "bf16":
        variant["x"] = "plain"
    _forward_case(H, NL, cell, nb, split, False, 7, 5, variant, seed=H + NL + nb + split)


# x streamed from global memory: the shortest T whose fp32 image (nb T H
# floats) exceeds the 48 KiB the kernels stage in LDS; both forward maps where
# the shape is valid for them (the K-split map starts at H = 32).
# (split, cell, H, NL, T, nb, variant)
_W = dict(I=9, state=True, bias=False, batch_first=True, x="wide")
_S = dict(I=1, state=False, bias=True, batch_first=False, x="plain")
_G = dict(I="H", state=True, bias=True, batch_first=True, x="idx")
_STREAM_FWD = [(1, 0, 64, 1, 193, 1, _W), (1, 0, 32, 2, 385, 1, _S), (1, 0, 32, 2, 193, 2, _G), (1, 0, 16, 4, 385, 2, _W),
               (2, 0, 64, 1, 193, 1, _S), (2, 0, 32, 2, 385, 1, _G), (2, 0, 32, 2, 193, 2, _W),
               (1, 1, 32, 2, 385, 1, _G), (1, 1, 16, 2, 385, 2, _S)]


@gpu
@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("split,cell,H,NL,T,nb,variant", _STREAM_FWD)
def test_forward_streamed_x(split, cell, H, NL, T, nb, variant, save):
    assert not _xlds(H, nb, T) and _xlds(H, nb, T - 1)
    _forward_case(H, NL, cell, nb, split, save, T, 3, variant, seed=H + T + nb + split, wscale=0.5)


def _backward_case(H, NL, cell, nb, split, T, B, name, seed, wscale=1.0, walk=False, twice=False, accum=False):
    mod = _ext.require()
    v = dict(_BWD_VARIANTS[name])
    final, seq = v.pop("final", True), v.pop("seq", True)
    need_dx, need_dh0, strided = v.pop("need_dx", True), v.pop("need_dh0", True), v.pop("strided", False)
    s = _inputs(H, NL, cell, B, T, v.pop("I"), seed, wscale=wscale, **v)
    hseq, hn, cn, act = mod.lstm_small_fwd(s.x, s.idx, s.w, s.h0, s.c0, H, NL, s.batch_first, True, True, 1, 1, cell)
    dev = hseq.device
    dout = dhn = dcn = None
    if seq:
        shape = (B, T) if s.batch_first else (T, B)
        if strided:
            dout = (torch.randn(*shape, H + 64, device=dev) * 0.1)[..., 32:32 + H]
            assert dout.stride(1) > H and not s.batch_first
        else:
            dout = torch.randn(*shape, H, device=dev) * 0.1
    if final:
        dhn = torch.randn(NL, B, H, device=dev) * 0.1
        dcn = torch.randn(NL, B, H, device=dev) * 0.1 if cell == 0 else None  # (gru_fused passes none)
    P = R.flat_offsets(s.w, NL)[-1][0]
    grid = mod.lstm_small_bwd_grid(H, NL, T, B, nb, split)
    if walk:
        assert split == 1 and 0 < grid < -(-B // nb), (grid, B, nb)
    buf = pre = None
    if accum:  # a view of exactly P elements inside a NaN-padded buffer, pre-filled
        buf = torch.full((P + 77,), float("nan"), device=dev)
        pre = torch.randn(P, device=dev)
        buf[33:33 + P] = pre
    args = (s.x, s.idx, s.w, s.h0, s.c0, hseq, act, dout, dhn, dcn, H, NL, s.batch_first, need_dx, need_dh0, nb, split)
    dparams, dx, dh0, dc0 = mod.lstm_small_bwd(*args, buf[33:33 + P] if accum else None, cell)
    torch.cuda.synchronize()
    assert dparams.shape == (P,)
    rp, budget, rdx, rdh0, rdc0 = R.backward(s.x_ref, s.w, s.h0, s.c0, hseq, act, _bm(dout, s.batch_first) if seq else None,
                                             dhn, dcn, H, NL, cell)
    got, ref, extra = dict(dparams=dparams), dict(dparams=rp), None
    if accum:
        assert dparams.data_ptr() == buf[33:].data_ptr()
        assert bool(torch.isnan(buf[:33]).all()) and bool(torch.isnan(buf[33 + P:]).all()), "padding touched"
        got["dparams"] = dparams.double() - pre.double()
        extra = 2.0 ** -22 * pre.double().abs()
    if need_dx:
        assert dx.shape == s.x.shape
        got["dx"], ref["dx"] = _bm(dx, s.batch_first), rdx
    else:
        assert dx is None
    if need_dh0:
        got["dh0"], ref["dh0"] = dh0, rdh0
        if cell == 0:  # the GRU has no cell state: dc0 is left unwritten
            got["dc0"], ref["dc0"] = dc0, rdc0
    else:
        assert dh0 is None and dc0 is None
    compare(_bwd_tag(split, cell, H, nb, T, walk), got, ref, budget, extra, worst=_worst)
    if twice:
        again = mod.lstm_small_bwd(*args, None, cell)
        for a, b in zip((dparams, dx, dh0, dc0), again):
            if a is not None and not (cell == 1 and a is dc0):
                assert torch.equal(a, b), "backward is not deterministic"


def _bwd_matrix():
    rows = []
    small = [(16, 1), (16, 4), (32, 2), (32, 4)]
    fams = [(1, 0, nb, small) for nb in (1, 2, 3)] + [(1, 0, 1, [(64, 1)])]
    fams += [(1, 1, 1, small + [(64, 1)]), (2, 0, 1, small + [(64, 1)])]
    for split, cell, nb, shapes in fams:
        for H, NL in shapes:
            for name in _BWD_VARIANTS:
                if name == "bf16" and (split == 2 or cell == 1):
                    continue  # refused (test_refusals) / fp32 only (ops.lstm.GRU.dtypes)
                rows.append(pytest.param(split, cell, nb, H, NL, name,
                                         id=f"{'unit' if split == 1 else 'rowsplit'}-{CELLS[cell]}-nb{nb}-H{H}x{NL}-{name}"))
    return rows


@gpu
@pytest.mark.parametrize("split,cell,nb,H,NL,name", _bwd_matrix())
def test_backward(split, cell, nb, H, NL, name):
    """Unit-group backward in its general form (LSTM with 1, 2, 3 sequences per
    workgroup, H = 64 and the GRU with one) and the row-split backward, every
    variant of what the caller may pass; B = 5 leaves one slot of the last
    workgroup empty at nb = 2 and nb = 3."""
    _backward_case(H, NL, cell, nb, split, 6 + (H + NL + nb) % 3, 5, name,
                   seed=7 * H + NL + 31 * nb + 1000 * split + 500 * cell + len(name))


@gpu
@pytest.mark.parametrize("H,NL,T,nb,split", [(64, 1, 193, 1, 1), (32, 2, 385, 1, 1), (32, 2, 193, 2, 1),
                                             (32, 1, 129, 3, 1), (32, 2, 385, 1, 2)])
@pytest.mark.parametrize("name", ["full"])
def test_backward_streamed_x(H, NL, T, nb, split, name):
    """The builds that read x from global memory every step.  Weights halved:
    the recurrent Jacobian contracts and the free-running carries of the
    kernel and of the reference do not drift apart over T steps."""
    assert not _xlds(H, nb, T) and _xlds(H, nb, T - 1)
    _backward_case(H, NL, 0, nb, split, T, 3, name, seed=H + T + nb + split, wscale=0.5)


@gpu
@pytest.mark.parametrize("split,cell,nb,H,NL", [(1, 0, 1, 32, 2), (1, 0, 3, 16, 4), (1, 1, 1, 32, 2), (2, 0, 1, 32, 4)])
def test_backward_grad_accum(split, cell, nb, H, NL):
    """grad_accum: the beta = 1 slab reduction adds the gradient to what the
    view holds and writes nothing outside its P elements."""
    _backward_case(H, NL, cell, nb, split, 7, 5, "full", seed=11 * H + nb + split, accum=True)


@gpu
@pytest.mark.parametrize("H,NL,nb", [(32, 4, 1), (32, 2, 3)])
def test_backward_persistent_walk(H, NL, nb):
    """grid < batch tiles: a workgroup carries its register dW over several
    tiles.  cap = the resident workgroups (the grid of a huge batch)."""
    mod = _ext.require()
    cap = mod.lstm_small_bwd_grid(H, NL, 4, 1 << 22, nb, 1)
    assert cap > 0
    B = nb * (cap + cap // 2) + 1
    assert mod.lstm_small_bwd_grid(H, NL, 4, B, nb, 1) == cap < -(-B // nb)
    _backward_case(H, NL, 0, nb, 1, 4, B, "full", seed=H + NL + nb, walk=True)


@gpu
@pytest.mark.parametrize("split,cell,nb,H,NL", [(1, 0, 1, 32, 2), (1, 0, 2, 32, 4), (1, 0, 3, 16, 1), (1, 0, 1, 64, 1),
                                                (1, 1, 1, 16, 4), (2, 0, 1, 32, 2)])
def test_backward_deterministic(split, cell, nb, H, NL):
    """The same backward twice: bit-identical dparams, dx, dh0, dc0."""
    _backward_case(H, NL, cell, nb, split, 7, 5, "full", seed=3 * H + nb, twice=True)


# ---------------------------------------------------------------------------
# refusals and routing
# ---------------------------------------------------------------------------
def _fwd_call(mod, s, H, NL, nb, split, cell, save=True):
    return mod.lstm_small_fwd(s.x, s.idx, s.w, s.h0, s.c0, H, NL, True, save, True, nb, split, cell)


def _bwd_call(mod, s, hseq, act, H, NL, nb, split, cell, need_dx=True):
    dhn = torch.ones(NL, hseq.shape[1], H, device=hseq.device)
    return mod.lstm_small_bwd(s.x, s.idx, s.w, s.h0, s.c0, hseq, act, None, dhn, None, H, NL, True, need_dx, True, nb,
                              split, None, cell)


_REFUSALS = ["gru fwd split 2", "gru bwd split 2", "gru bwd nb 2", "ks fwd H 16", "bwd nb 2 H 64", "rowsplit nb 2",
             "bf16 rowsplit", "bf16 fwd past LDS", "bf16 bwd past LDS", "dx with idx"]


@gpu
@pytest.mark.parametrize("what", _REFUSALS)
def test_refusals(what):
    """Configurations the host code rejects before any launch raise, and the
    valid launch of the same operands afterwards passes."""
    mod = _ext.require()
    cell = 1 if what.startswith("gru") else 0
    H, NL = {"ks fwd H 16": (16, 2), "bwd nb 2 H 64": (64, 1)}.get(what, (32, 2))
    T = 385 if "past LDS" in what else 7
    xk = "bf16" if "bf16" in what else "idx" if "idx" in what else "plain"
    s = _inputs(H, NL, cell, 5, T, 9, seed=len(what), x=xk)
    s32 = s
    if "past LDS" in what:  # the forward takes this length in fp32 only; its saved tensors serve the bf16 backward
        s32 = copy.copy(s)
        s32.x = s.x.float()
    hseq, _, _, act = _fwd_call(mod, s32, H, NL, 1, 1, cell)
    bad_fwd = {"gru fwd split 2": (1, 2), "ks fwd H 16": (1, 2), "bf16 fwd past LDS": (1, 1)}
    bad_bwd = {"gru bwd split 2": (1, 2), "gru bwd nb 2": (2, 1), "bwd nb 2 H 64": (2, 1), "rowsplit nb 2": (2, 2),
               "bf16 rowsplit": (1, 2), "bf16 bwd past LDS": (1, 1), "dx with idx": (1, 1)}
    with pytest.raises(RuntimeError):
        if what in bad_fwd:
            _fwd_call(mod, s, H, NL, *bad_fwd[what], cell)
        else:
            _bwd_call(mod, s, hseq, act, H, NL, *bad_bwd[what], cell)
    torch.cuda.synchronize()
    # ... and the nearest valid launch
    ok = s32 if "past LDS" in what else s
    out = _bwd_call(mod, ok, hseq, act, H, NL, 1, 1, cell, need_dx="idx" not in what)
    ref = R.backward(ok.x_ref, ok.w, ok.h0, ok.c0, hseq, act, None, torch.ones(NL, 5, H, device="cuda"), None, H, NL, cell)
    compare("refusal, then valid", dict(dparams=out[0], dh0=out[2]), dict(dparams=ref[0], dh0=ref[3]), ref[1])


@gpu
@pytest.mark.parametrize("tune,B,want_fwd,want_bwd", [
    (dict(split_fwd=2), 8, (1, 2), (1, 0)),
    (dict(split_bwd=2), 8, (1, 0), (1, 2)),
    (dict(nb_bwd=2), 8, (1, 0), (2, 0)),
    (dict(nb_bwd=3), 8, (1, 0), (3, 0)),
    (dict(), 1024, (1, 0), (1, 0)),
    (dict(), 1025, (1, 2), (1, 0)),
])
def test_tune_reaches_bindings(monkeypatch, tune, B, want_fwd, want_bwd):
    """PDRNN_TUNE split_fwd / split_bwd / nb_bwd and the B > 1024 rule arrive
    at the bindings as (nb, split) through ops.lstm.lstm_forward and its
    autograd node, for the training and the inference call."""
    mod = _ext.require()
    set_tune(monkeypatch, nb_fwd=None, split_fwd=None, nb_bwd=None, split_bwd=None)
    set_tune(monkeypatch, **tune)
    seen = []
    real_fwd, real_bwd = mod.lstm_small_fwd, mod.lstm_small_bwd

    def spy_fwd(*a, **k):
        seen.append(("fwd", a[8], a[10], a[11]))
        return real_fwd(*a, **k)

    def spy_bwd(*a, **k):
        seen.append(("bwd", None, a[15], a[16]))
        return real_bwd(*a, **k)
    monkeypatch.setattr(mod, "lstm_small_fwd", spy_fwd)
    monkeypatch.setattr(mod, "lstm_small_bwd", spy_bwd)
    H, NL, T, I = 32, 2, 6, 9
    s = _inputs(H, NL, 0, B, T, I, seed=B, state=False)
    ws = [t.clone().requires_grad_() for t in s.w]
    out, hn, cn = lstm_ops.lstm_forward(s.x, ws, hidden=H, num_layers=NL, batch_first=True)
    (out.sum() + cn.sum()).backward()
    with torch.no_grad():
        out_i, hn_i, cn_i = lstm_ops.lstm_forward(s.x, s.w, hidden=H, num_layers=NL, batch_first=True)
    torch.cuda.synchronize()
    assert seen == [("fwd", True) + want_fwd, ("bwd", None) + want_bwd, ("fwd", False) + want_fwd], seen
    rh, _, rhn, rcn = R.forward(s.x_ref, s.w, None, None, H, NL)
    for o, h, c in ((out, hn, cn), (out_i, hn_i, cn_i)):
        compare("operator", dict(out=o.detach(), hn=h.detach(), cn=c.detach()), dict(out=rh[NL - 1], hn=rhn, cn=rcn))
    grads = torch.cat([w.grad.reshape(-1) for w in ws])
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
