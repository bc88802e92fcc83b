"""GPU: the host code that turns the large-H recurrence kernels and the
in-tree GEMMs into an nn.LSTM / nn.GRU layer (ops/lstm_large.py: _LargeLayer,
_backward_gemms16, _weight_grads, _PipelinedStack, _StackStates,
_final_states, the shadow builders; ops/gru_large.py: _gru_shadows, _db_hh,
_backward_gemms16), per element against the fp64 reference of
tests/_layer_ref.py.

Capture.  The public modules (models.rnn.LSTM / GRU) run under
PDRNN_KERNELS=hip-strict with recording wrappers on lstm_large_fwd /
lstm_large_bwd / lstm_rows_fwd_range / lstm_rows_bwd_range: every call's
arguments and results are kept (references, read after a device
synchronize) and the call goes through unchanged.  The reference is built
from what the recurrence received and returned, so none of its rounding
enters; what is compared is the host code alone:

* bitwise (torch.equal): the weight operands against the _large_ref packing
  of the parameters rounded once to the compute dtype (the GRU's zero blocks
  exactly zero), hn / cn against the last processed step of the captured
  hseq / sseq in [layer*ndir + d] order, the top layer's dout and every
  layer's dhn / dcn against the caller's gradients, dh0 / dc0 against the
  captured fp32 values cast once, None for a state without a gradient;
* bounded (_layer_ref.ratio <= 1, the bound of _gemm_ref.bound_ratio):
  |got - ref| <= (K + S + 1) 2^-23 (|A| |B|) (+ u16 |ref| for a 16-bit
  result), the folded bias and the old value of an accumulated gradient one
  more term each, for xp (layer l + 1's from layer l's captured hseq), dx
  (layer l's dout is layer l + 1's dx), dW_ih, dW_hh, db_ih, db_hh.
  S is the largest split count the wrapper can choose: min(16, K / 1024) for
  gemm16 (ops/gemm.py:_splitk), min(128, K / 128) for gemm_f32 (_splitk_f32),
  the number of pairs for a library product (one fp32 add per further pair).

Two library fallbacks round once more than that bound assumes, and get
exactly that term:
* linear16 off the in-tree GEMM is addmm(bias.to(16 bit), ...): + u16 |bias|;
* mm_nk16 off the in-tree GEMM with two directions rounds the first product
  to 16 bits before addmm_ adds the second: + u16 |first| (the
  rounded_first64 of _gemm_ref.assert_within_ulp16; the K 2^-23 |A| |B| term
  stays because these operands, unlike test_linear_routes_exact's, are not
  dyadic).

Every case asserts the native GEMM calls it made (gemm16 / gemm_f32 /
col_sum, counted as in test_gpu_gemm_f32_exact.py), whether the library ran,
and which Function ran (_PipelinedStack or _LargeLayer).

Worst |got - ref| / bound per route and quantity on an MI355X when this file
was written (16-bit results: a correct rounding alone reaches 1.0 of the
u16 |ref| term, so those sit just below 1):

    route      xp      dx      dW_ih   dW_hh   db_ih   db_hh
    gemm16     0.9921  0.9215  0.0093  0.0190  -       -
    gemm_f32   0.1231  0.0076  0.2191  0.2236  0.1182  0.1182
    col_sum    -       -       -       -       0.0185  0.1161
    library    0.9318  0.6359  0.1821  0.1752  -       -
    fill       -       -       -       0 (exact zero, or old + 0 in direct mode)

The 45 cases take 4 s together.
"""
import collections

import pytest
import torch

import _gemm_ref as GR
import _layer_ref as LR
from _tune import set_tune
from test_gpu_lstm_pipeline import _count_pipelined

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.rnn import GRU, LSTM
from pytorch_distributed_rnn_amd.ops import gemm as G
from pytorch_distributed_rnn_amd.ops import gradsink, gru_large, lstm_large

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
CELL = {0: (LSTM, lstm_large.LSTM), 1: (GRU, gru_large.GRU)}
RECURRENCE = ("lstm_large_fwd", "lstm_large_bwd", "lstm_rows_fwd_range", "lstm_rows_bwd_range")

_worst = collections.defaultdict(float)  # (route, quantity) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nworst |got - ref| / bound per route and quantity")
        for (route, name), v in sorted(_worst.items()):
            print(f"RATIO {route:9s} {name:6s} {v:.4f}")


def _s16(K):
    return min(16, max(1, K // (64 * 16)))     # ops/gemm.py:_splitk


def _s32(K):
    return min(128, max(1, K // (16 * 8)))     # ops/gemm.py:_splitk_f32


# ---------------------------------------------------------------- capture
class _Counting:
    """The native module with its GEMM entry points counted (the proxy of
    test_gpu_gemm_f32_exact.py)."""

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


class _Capture:
    def __init__(self, monkeypatch):
        mod = _ext.require()
        self.calls = {n: [] for n in RECURRENCE}
        for name in RECURRENCE:
            monkeypatch.setattr(mod, name, self._recording(name, getattr(mod, name)))
        self.gemm = _Counting(mod)
        n16, nf32 = G._native, G._native_f32
        monkeypatch.setattr(G, "_native", lambda t: self.gemm if n16(t) is not None else None)
        monkeypatch.setattr(G, "_native_f32", lambda t: self.gemm if nf32(t) is not None else None)
        self.library = 0
        for name in ("mm", "addmm"):
            monkeypatch.setattr(torch, name, self._library(getattr(torch, name)))
        self.layer = []
        orig = lstm_large._LargeLayer.apply

        def apply(*a):
            self.layer.append(a[3][0])
            return orig(*a)
        monkeypatch.setattr(lstm_large._LargeLayer, "apply", apply)

    def _recording(self, name, fn):
        def call(*a):
            out = fn(*a)
            self.calls[name].append((a, out))
            return out
        return call

    def _library(self, fn):
        def call(*a, **k):
            self.library += 1
            return fn(*a, **k)
        return call


class _Layer:
    """One layer's recurrence operands and results, on the CPU, in the layout
    of lstm_large_fwd / lstm_large_bwd whichever binding ran."""


def _cpu(t):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_cpu(v) for v in t]
    return t.detach().cpu()


def _layers(cap, L):
    """Per layer, from the recorded calls (after a synchronize)."""
    torch.cuda.synchronize()
    out = []
    if cap.calls["lstm_large_fwd"]:
        assert not cap.calls["lstm_rows_fwd_range"] and not cap.calls["lstm_rows_bwd_range"]
        fwd, bwd = cap.calls["lstm_large_fwd"], cap.calls["lstm_large_bwd"]
        assert len(fwd) == len(bwd) == L
        for a, (hseq, sseq, acts) in fwd:
            y = _Layer()
            y.xp, y.w, y.h0, y.s0, y.H, y.mask, y.tile, y.cell = _cpu(a[0]), _cpu(a[1]), _cpu(a[2]), _cpu(a[3]), *a[4:]
            y.hseq, y.sseq = _cpu(hseq), _cpu(sseq)
            mine = [(b, r) for b, r in bwd if b[5].data_ptr() == acts.data_ptr()]
            assert len(mine) == 1, "one BPTT per layer, on the forward's acts"
            b, (dgates, dh0, dc0) = mine[0]
            assert b[4].data_ptr() == sseq.data_ptr() and tuple(b[7:]) == tuple(a[4:])
            assert (b[6] is None) == (a[3] is None) and (b[6] is None or b[6].data_ptr() == a[3].data_ptr())
            y.dout, y.dhn, y.dcn, y.wt = _cpu(b[0]), _cpu(b[1]), _cpu(b[2]), _cpu(b[3])
            y.dgates, y.dh0, y.dc0 = _cpu(dgates), _cpu(dh0), _cpu(dc0)
            out.append(y)
        # the BPTTs ran top layer first
        assert [b[5].data_ptr() for b, _ in bwd] == [r[2].data_ptr() for _, r in reversed(fwd)]
        return out
    fwd, bwd = cap.calls["lstm_rows_fwd_range"], cap.calls["lstm_rows_bwd_range"]
    assert not cap.calls["lstm_large_bwd"]
    order = []
    for a, _ in fwd:
        if a[4].data_ptr() not in order:
            order.append(a[4].data_ptr())
    assert len(order) == L
    for ptr in order:
        f = sorted((a for a, _ in fwd if a[4].data_ptr() == ptr), key=lambda a: a[7])
        y = _Layer()
        a = f[0]
        T = a[4].shape[0]
        y.chunks = [(c[7], c[8]) for c in f]
        assert y.chunks[0][0] == 0 and y.chunks[-1][1] == T and all(p[1] == q[0] for p, q in zip(y.chunks, y.chunks[1:]))
        for c in f:  # one set of full-length tensors and operands per layer
            assert all((c[k] is None and a[k] is None) or c[k].data_ptr() == a[k].data_ptr() for k in (1, 2, 3, 4, 5, 6))
            assert c[9] == a[9] and c[0].shape[0] == c[8] - c[7]
        y.xp = torch.cat([_cpu(c[0]) for c in f], 0)
        y.w, y.H, y.mask, y.cell = [_cpu(a[1])], a[1].shape[1], 0, a[9]
        y.h0 = _cpu(a[2])[None] if a[2] is not None else None
        y.s0 = _cpu(a[3])[None] if a[3] is not None else None
        y.hseq, y.sseq = _cpu(a[4]), _cpu(a[5])[None]
        b = sorted((b for b, _ in bwd if b[5].data_ptr() == a[6].data_ptr()), key=lambda b: b[11])
        assert [(c[11], c[12]) for c in b] == y.chunks, "the BPTT ran the forward's chunks"
        last, first = b[-1], b[0]
        for c in b:
            assert c[4].data_ptr() == a[5].data_ptr() and c[13] == a[9]
            assert all(c[k].data_ptr() == first[k].data_ptr() for k in (3, 7, 8, 9, 10))
            assert (c[6] is None) == (a[3] is None) and (c[6] is None or c[6].data_ptr() == a[3].data_ptr())
            if c is not last:  # a lower chunk starts from what the chunk above left
                assert c[1].data_ptr() == c[8].data_ptr() and (c[2] is None or c[2].data_ptr() == c[9].data_ptr())
        y.dout = torch.cat([_cpu(c[0]) for c in b], 0) if first[0] is not None else None
        y.dhn = _cpu(last[1])[None] if last[1] is not None else None
        y.dcn = _cpu(last[2])[None] if last[2] is not None else None
        y.wt = [_cpu(first[3])]
        y.dgates, y.dh0, y.dc0 = _cpu(first[7])[None], _cpu(first[8])[None], _cpu(first[9])[None]
        out.append(y)
    return out


# ---------------------------------------------------------------- one case
def _names(l, d):
    sfx = f"_l{l}" + ("_reverse" if d else "")
    return ["weight_ih" + sfx, "weight_hh" + sfx, "bias_ih" + sfx, "bias_hh" + sfx]


def _preload(m, flat, seed):
    """Every .grad preloaded with dyadic values: views of one flat buffer
    (b_ih / b_hh adjacent) or tensors of their own."""
    g = GR.gen(seed)
    ps = list(m.parameters())
    old = {}
    buf = torch.empty(sum(p.numel() for p in ps), device="cuda") if flat else None
    off = 0
    for p in ps:
        o64 = (GR.dyadic(p.numel(), 1, g) * 8).view(p.shape)
        if flat:
            p.grad = buf[off:off + p.numel()].view(p.shape)
            p.grad.copy_(o64)
            off += p.numel()
        else:
            p.grad = o64.float().cuda()
        old[id(p)] = (o64, p.grad, p.grad.data_ptr(), p.grad.untyped_storage().data_ptr())
    bi, bh = getattr(m, "bias_ih_l0", None), getattr(m, "bias_hh_l0", None)
    if bi is not None:  # the condition of _add_bias_sinks' single add
        assert (bh.grad.data_ptr() == bi.grad.data_ptr() + 4 * bi.numel() and
                bh.grad.untyped_storage().data_ptr() == bi.grad.untyped_storage().data_ptr()) == bool(flat)
    return old


def _run(monkeypatch, cell, dtype, H, L, ndir, B, T, I, *, bias=True, state=True, state_dtype=None, direct=None,
         pipelined=False, seed=0):
    """Forward + backward of the public module with everything captured, then
    every assertion of this file; returns (capture, layers)."""
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    lstm = cell == 0
    torch.manual_seed(1000 * cell + 10 * H + B + T + seed)
    m = CELL[cell][0](I, H, L, bias=bias, bidirectional=ndir == 2).cuda()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith("bias"):
                p.copy_(torch.randn_like(p) * 0.5)
    sdt = state_dtype or dtype
    x = torch.randn(T, B, I, device="cuda").to(dtype).requires_grad_()
    h0 = (torch.randn(L * ndir, B, H, device="cuda") * 0.5).to(sdt).requires_grad_() if state else None
    # the LSTM's c0 is given but needs no gradient in the bidirectional cases
    c0 = (torch.randn(L * ndir, B, H, device="cuda") * 0.5).to(sdt).requires_grad_(ndir == 1) if state and lstm else None
    old = _preload(m, direct == "flat", seed + 5) if direct else None

    cap = _Capture(monkeypatch)
    piped = _count_pipelined(monkeypatch, CELL[cell][1])
    with gradsink.direct_grads(bool(direct)):
        if lstm:
            out, (hn, cn) = m(x, (h0, c0) if state else None)
        else:
            out, hn = m(x, h0)
            cn = None
        g = torch.randn_like(out)
        ghn = torch.randn_like(hn)
        gcn = torch.randn_like(cn) if lstm else None
        torch.autograd.backward([out, hn] + ([cn] if lstm else []), [g, ghn] + ([gcn] if lstm else []))
    ys = _layers(cap, L)

    # which Function ran
    assert len(piped) == (1 if pipelined else 0) and cap.layer == ([] if pipelined else [CELL[cell][1]] * L)

    gates, xcols, hh_blocks = LR.CELLS[cell]
    want = collections.Counter()
    lib = 0
    f32 = dtype == FP32
    u16 = 0.0 if f32 else LR.U16[dtype]
    mask = 2 if ndir == 2 else 0
    last = [T - 1, 0]
    out_c, hn_c, cn_c = _cpu(out), _cpu(hn), _cpu(cn)
    assert out.dtype == dtype and hn.dtype == dtype and torch.equal(out_c, ys[-1].hseq)

    def note(route, name, r):
        _worst[(route, name)] = max(_worst[(route, name)], r)
        assert r <= 1.0, f"{name} on {route}: error / bound = {r:.3f}"

    for l, y in enumerate(ys):
        what = f"layer {l}"
        assert (y.H, y.mask, y.cell) == (H, mask, cell) and y.hseq.shape == (T, B, ndir * H)
        I_l = I if l == 0 else ndir * H
        x_l = _cpu(x) if l == 0 else ys[l - 1].hseq
        ps = [[getattr(m, n, None) for n in _names(l, d)] for d in range(ndir)]
        rounded = [(_cpu(w_ih).to(dtype), _cpu(w_hh).to(dtype), _cpu(b_ih), _cpu(b_hh)) for w_ih, w_hh, b_ih, b_hh in ps]
        pk = LR.packed(cell, rounded, H)

        # ---- operands of the recurrence, bitwise
        for d in range(ndir):
            assert y.w[d].dtype == dtype and torch.equal(y.w[d], pk.w[d]), f"{what}: W_hh interleaved, direction {d}"
            assert y.wt[d].dtype == dtype and torch.equal(y.wt[d], pk.wt[d]), f"{what}: W_hh^T, direction {d}"
            if not lstm:  # the n_x rows of the recurrent stack
                assert not y.w[d].view(H, 4, H)[:, 2].any() and not y.wt[d][:, 2 * H:3 * H].any()
        sl = slice(l * ndir, (l + 1) * ndir)
        if state:
            assert y.h0.dtype == dtype and torch.equal(y.h0, _cpu(h0)[sl].to(dtype)), f"{what}: h0"
            assert y.s0.dtype == FP32 and torch.equal(y.s0, _cpu(c0 if lstm else h0)[sl].float()), f"{what}: fp32 state"
        else:
            assert y.h0 is None and y.s0 is None

        # ---- input projection
        if f32:
            route, extra = "gemm_f32", None
            want["gemm_f32"] += 0 if pipelined and l else 1  # (the pipeline's chunked ones are counted below)
        elif GR.gemm16_supported(T * B, ndir * 4 * H, I_l, 0, False, False, True):
            route, extra = "gemm16", None
            want["gemm16"] += 1
        else:  # addmm(bias.to(16 bit), x, W^T): the bias is rounded before it is added
            route, extra = "library", u16 * pk.bias_mag
            lib += 1
        note(route, "xp", LR.ratio(y.xp.reshape(T * B, -1), LR.xp(x_l, pk), 1, extra))

        # ---- final states, bitwise
        for d in range(ndir):
            assert torch.equal(hn_c[l * ndir + d], y.hseq[last[d], :, d * H:(d + 1) * H]), f"{what}: hn[{l * ndir + d}]"
            if lstm:
                assert cn_c.dtype == dtype and torch.equal(cn_c[l * ndir + d], y.sseq[d, last[d]].to(dtype)), f"{what}: cn"

        # ---- gradients entering the BPTT, bitwise
        if l == L - 1:
            assert y.dout.dtype == dtype and torch.equal(y.dout, _cpu(g).to(dtype)), "top layer's dout"
        assert y.dhn.dtype == FP32 and torch.equal(y.dhn, _cpu(ghn)[sl].float()), f"{what}: dhn"
        if lstm:
            assert y.dcn.dtype == FP32 and torch.equal(y.dcn, _cpu(gcn)[sl].float()), f"{what}: dcn"
        else:
            assert y.dcn is None
        # ---- gradients of the initial state: the captured fp32 values, cast once
        if state:
            assert h0.grad.dtype == sdt and torch.equal(_cpu(h0.grad)[sl], y.dh0.to(sdt)), f"{what}: dh0"
            if lstm and c0.requires_grad:
                assert c0.grad.dtype == sdt and torch.equal(_cpu(c0.grad)[sl], y.dc0.to(sdt)), f"{what}: dc0"
            elif lstm:
                assert c0.grad is None

        # ---- weight, bias and input gradients
        lg = LR.grads(cell, y.dgates, y.hseq, y.h0, x_l, pk.wih, H)
        TB = T * B
        Kx = xcols * H
        dx_got = (_cpu(x.grad) if l == 0 else ys[l - 1].dout).reshape(TB, I_l)
        assert dx_got.dtype == dtype
        if f32:
            want["gemm_f32"] += 0 if pipelined else 1  # (the pipeline's are counted below)
            note("gemm_f32", "dx", LR.ratio(dx_got, lg.dx, _s32(ndir * Kx)))
        elif GR.gemm16_supported(TB, I_l, Kx, Kx if ndir == 2 else 0, False, True, True):
            want["gemm16"] += 1
            note("gemm16", "dx", LR.ratio(dx_got, lg.dx, 1))
        else:  # mm then addmm_: the first direction's product is rounded to 16 bits before the second is added
            lib += 1
            note("library", "dx", LR.ratio(dx_got, lg.dx, ndir, u16 * lg.dx_parts[0].ref.abs() if ndir == 2 else None))
        for d in range(ndir):
            K_hh = (T if state else T - 1) * B
            routes = {}
            if f32:
                nb = len(hh_blocks) if K_hh else 0
                want["gemm_f32"] += nb + 1
                want["col_sum"] += 0 if lstm else 1
                routes = {"dW_ih": ("gemm_f32", _s32(TB)), "dW_hh": ("gemm_f32", _s32(K_hh)),
                          "db_ih": ("gemm_f32", _s32(TB)), "db_hh": ("gemm_f32" if lstm else "col_sum", _s32(TB))}
            else:
                want["col_sum"] += 0 if (lstm and direct and not bias and K_hh) else 1
                routes["db_ih"] = routes["db_hh"] = ("col_sum", 1)
                if GR.gemm16_supported(gates * H, I_l, TB, 0, True, True, False):
                    want["gemm16"] += 1
                    routes["dW_ih"] = ("gemm16", _s16(TB))
                else:
                    lib += 1
                    routes["dW_ih"] = ("library", 1)
                if lstm:  # K segments: the shifted steps, then the h0 pairing
                    K1, K2 = ((T - 1) * B, B if state else 0) if T > 1 else (B if state else 0, 0)
                else:     # one product against the concatenated h_prev (zero rows without a state)
                    K1, K2 = TB, 0
                if K1 == 0:
                    routes["dW_hh"] = ("fill", 0)
                elif GR.gemm16_supported(4 * H, H, K1, K2, True, True, False):
                    want["gemm16"] += 1
                    routes["dW_hh"] = ("gemm16", _s16(K1 + K2))
                else:
                    lib += 1
                    routes["dW_hh"] = ("library", 2 if K2 else 1)
            for k, p in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), ps[d]):
                if p is None:
                    assert not bias and k.startswith("db")
                    continue
                route, S = routes[k]
                exp = lg.params[d][k]
                assert p.grad is not None and p.grad.dtype == FP32 and p.grad.shape == exp.ref.shape, f"{what}: {k}"
                if direct:
                    o64, gt, ptr, sptr = old[id(p)]
                    assert p.grad is gt and p.grad.data_ptr() == ptr and p.grad.untyped_storage().data_ptr() == sptr, \
                        f"{what}: {k}: .grad replaced, not accumulated in place"
                    exp = LR.plus(exp, o64)
                    if k == "dW_hh" and K_hh == 0:
                        assert torch.equal(_cpu(p.grad).double(), o64), f"{what}: {k}: old + an exact zero"
                elif k == "dW_hh" and K_hh == 0:
                    assert not _cpu(p.grad).any(), f"{what}: {k} is an exact zero fill"
                note(route, k, LR.ratio(_cpu(p.grad), exp, S))

    if pipelined:
        C = len(ys[0].chunks)
        assert all(y.chunks == ys[0].chunks for y in ys)
        want["gemm_f32"] += 2 * (L - 1) * C + 1   # chunked projections up and dX down, layer 0's dX
    assert dict(cap.gemm.calls) == {k: v for k, v in want.items() if v}, \
        f"native GEMM calls {dict(cap.gemm.calls)}, expected {dict(want)}"
    assert (cap.library > 0) == (lib > 0), f"{cap.library} library calls, {lib} library products expected"
    return cap, ys


# ---------------------------------------------------------------- the cases
CELLS = [pytest.param(0, id="lstm"), pytest.param(1, id="gru")]
BITS16 = [pytest.param(BF16, id="bf16"), pytest.param(FP16, id="fp16")]


@pytest.mark.parametrize("dtype", BITS16)
@pytest.mark.parametrize("cell", CELLS)
def test_a_two_layers_every_product_on_gemm16(monkeypatch, cell, dtype):
    """H 128, 2 layers, B 64, T 3, I 64, fp32 initial state: every product on
    gemm16 -- the LSTM's dW_hh as two K segments (K1 = 128, K2 = 64), the GRU's
    against a concatenated h_prev -- and no library call."""
    cap, _ = _run(monkeypatch, cell, dtype, 128, 2, 1, 64, 3, 64, state_dtype=FP32)
    assert cap.library == 0 and cap.gemm.calls["gemm16"] == 8 and cap.gemm.calls["col_sum"] == 2
    assert "gemm_f32" not in cap.gemm.calls


@pytest.mark.parametrize("dtype", BITS16)
@pytest.mark.parametrize("cell", CELLS)
def test_b_bidirectional_library_fallbacks(monkeypatch, cell, dtype):
    """H 64, 2 layers, bidirectional, B 5, T 3, I 24: 15 rows, so the weight
    gradients and layer 0's projection run on the library; the reverse
    direction's shift (+1) and edge step (T - 1); both directions' dX in one
    gemm16 call (two K segments)."""
    cap, _ = _run(monkeypatch, cell, dtype, 64, 2, 2, 5, 3, 24)
    assert cap.library > 0 and cap.gemm.calls["gemm16"] == 3   # layer 1's projection, both layers' dX


@pytest.mark.parametrize("dtype", BITS16)
@pytest.mark.parametrize("cell", CELLS)
def test_c_no_bias_no_state(monkeypatch, cell, dtype):
    """H 128, 1 layer, bidirectional, B 64, T 2, I 64: one pair only, no bias
    parameters (a zero folded bias), no state gradients."""
    cap, _ = _run(monkeypatch, cell, dtype, 128, 1, 2, 64, 2, 64, bias=False, state=False)
    assert cap.library == 0


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("dtype", BITS16)
@pytest.mark.parametrize("cell", CELLS)
def test_d_single_step_16bit(monkeypatch, cell, dtype, state):
    """T 1, H 128, bidirectional, B 5, I 9: dW_hh is the h0 pairing alone, an
    exact zero fill without a state; every product on the library, dX of two
    directions as mm + addmm_."""
    cap, _ = _run(monkeypatch, cell, dtype, 128, 1, 2, 5, 1, 9, state=state)
    assert "gemm16" not in cap.gemm.calls and cap.library > 0


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("pipe", [True, False])
@pytest.mark.parametrize("cell", CELLS)
def test_d_single_step_fp32(monkeypatch, cell, pipe, state):
    """T 1, H 128, 2 layers, fp32, B 5, I 9, through the pipelined stack (its
    chunks clamp to one) and layer by layer."""
    if not pipe:
        set_tune(monkeypatch, large_pipe="0")
    _, ys = _run(monkeypatch, cell, FP32, 128, 2, 1, 5, 1, 9, state=state, pipelined=pipe)
    assert not pipe or ys[0].chunks == [(0, 1)]


def test_e_direct_gradients_16bit(monkeypatch):
    """Case A's LSTM in direct-gradient mode: every .grad preloaded, the result
    is old + reference within the bound in the same storage (had autograd
    delivered as well, it would be old + 2 reference)."""
    cap, _ = _run(monkeypatch, 0, BF16, 128, 2, 1, 64, 3, 64, state_dtype=FP32, direct="own")
    assert cap.library == 0 and cap.gemm.calls["gemm16"] == 8 and cap.gemm.calls["col_sum"] == 2


def test_e_direct_gradients_16bit_single_step_without_state(monkeypatch):
    """Direct mode, T 1, no state: no pair to accumulate, so the layer falls
    back to autograd delivery -- still old + reference, dW_hh old + exact 0."""
    _run(monkeypatch, 0, BF16, 128, 2, 1, 64, 1, 64, state=False, direct="own")


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("pipe", [True, False])
@pytest.mark.parametrize("cell", CELLS)
def test_f_fp32_stack_chunked(monkeypatch, cell, pipe, state):
    """H 128, 2 layers, fp32, B 17, T 5, I 9, large_chunks 3 (steps 0-1, 1-3,
    3-5): the pipelined stack and, with large_pipe 0, the layer path; the
    narrow-input padded_cols product, the row-sum bias gradient, the GRU's
    _db_hh."""
    set_tune(monkeypatch, large_chunks="3", **({} if pipe else {"large_pipe": "0"}))
    _, ys = _run(monkeypatch, cell, FP32, 128, 2, 1, 17, 5, 9, state=state, pipelined=pipe)
    assert not pipe or ys[0].chunks == [(0, 1), (1, 3), (3, 5)]


@pytest.mark.parametrize("grads", ["flat", "own"])
def test_f_fp32_pipeline_direct_gradients(monkeypatch, grads):
    """The LSTM pipeline in direct mode: gradients accumulated by the GEMM
    epilogues; "flat": b_ih / b_hh adjacent views of one buffer (the single-add
    branch of _add_bias_sinks), "own": tensors of their own (one add each)."""
    set_tune(monkeypatch, large_chunks="3")
    _run(monkeypatch, 0, FP32, 128, 2, 1, 17, 5, 9, direct=grads, pipelined=True)


@pytest.mark.parametrize("H", [128, 192])
@pytest.mark.parametrize("cell", CELLS)
def test_g_fp32_bidirectional_layer(monkeypatch, cell, H):
    """fp32, 1 layer, bidirectional, B 5, T 3, I 9: the layer path with the two
    directions' dX as two K segments of one gemm_f32 call; H 192 leaves the
    row-owning kernels."""
    assert bool(_ext.require().lstm_rows_range_supported(H)) == (H == 128)
    _run(monkeypatch, cell, FP32, H, 1, 2, 5, 3, 9)


def test_h_padded_hidden_size(monkeypatch):
    """LSTM H 100 (zero-padded to 128), 2 layers, fp32, B 6, T 4, I 9: the
    captured hseq / dgates are exactly zero on the padded units, and the
    module's unpadded gradients meet the bound against the reference built
    from the unpadded slices."""
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    H, Hp, L, B, T, I = 100, 128, 2, 6, 4, 9
    torch.manual_seed(77)
    m = LSTM(I, H, L).cuda()
    x = torch.randn(T, B, I, device="cuda", requires_grad=True)
    h0 = (torch.randn(L, B, H, device="cuda") * 0.5).requires_grad_()
    c0 = (torch.randn(L, B, H, device="cuda") * 0.5).requires_grad_()
    cap = _Capture(monkeypatch)
    piped = _count_pipelined(monkeypatch, lstm_large.LSTM)
    out, (hn, cn) = m(x, (h0, c0))
    g, ghn, gcn = torch.randn_like(out), torch.randn_like(hn), torch.randn_like(cn)
    torch.autograd.backward([out, hn, cn], [g, ghn, gcn])
    ys = _layers(cap, L)
    assert len(piped) == 1 and not cap.layer and out.shape == (T, B, H)
    assert dict(cap.gemm.calls) == {"gemm_f32": 1 + 2 * len(ys[0].chunks) + 2 * 2 + 1}
    unpad = lambda t: t.reshape(*t.shape[:-1], -1, Hp)[..., :H].reshape(*t.shape[:-1], -1)
    for l, y in enumerate(ys):
        assert y.H == Hp
        for name in ("hseq", "sseq", "dgates", "dh0", "dc0"):
            t = getattr(y, name)
            assert not t.reshape(*t.shape[:-1], -1, Hp)[..., H:].any(), f"layer {l}: {name} on the padded units"
        assert torch.equal(unpad(y.hseq[T - 1]), _cpu(hn)[l]) and torch.equal(unpad(y.sseq[0, T - 1]), _cpu(cn)[l])
        assert torch.equal(_cpu(h0.grad)[l], unpad(y.dh0[0])) and torch.equal(_cpu(c0.grad)[l], unpad(y.dc0[0]))
        ps = [getattr(m, n) for n in _names(l, 0)]
        pk = LR.packed(0, [tuple(_cpu(p) for p in ps)], H)
        x_l = _cpu(x) if l == 0 else unpad(ys[l - 1].hseq)
        lg = LR.grads(0, unpad(y.dgates), unpad(y.hseq), unpad(y.h0), x_l, pk.wih, H)
        for k, p in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), ps):
            r = LR.ratio(_cpu(p.grad), lg.params[0][k], _s32(T * B))
            _worst[("gemm_f32", k)] = max(_worst[("gemm_f32", k)], r)
            assert r <= 1.0, f"layer {l}: {k}: error / bound = {r:.3f}"
        dx_got = _cpu(x.grad).reshape(T * B, I) if l == 0 else unpad(ys[l - 1].dout).reshape(T * B, H)
        r = LR.ratio(dx_got, lg.dx, _s32(4 * Hp))
        _worst[("gemm_f32", "dx")] = max(_worst[("gemm_f32", "dx")], r)
        assert r <= 1.0, f"layer {l}: dx: error / bound = {r:.3f}"
    assert torch.equal(_cpu(out), unpad(ys[-1].hseq)) and torch.equal(ys[-1].dout[..., :H], _cpu(g))
    assert not ys[-1].dout[..., H:].any()
