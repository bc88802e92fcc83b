"""lstm_large_fwd / lstm_large_bwd (csrc/kernels/lstm_large.hip,
lstm_rows_f32.hip) against the fp64 reference of tests/_large_ref.py, per
element, on every kernel path of the large-H recurrence.

The reference is teacher-forced (see _large_ref.py): each step is evaluated
in fp64 on the kernel's own stored result of the step before it, so kernel and
reference see identical inputs at every step and the only differences left are
the step's own fp32 arithmetic and the rounding of what it stores.  Bound, for
every element of every returned tensor:

    |kernel - ref| <= 2e-5 + (1e-4 + r) |ref|

2e-5 / 1e-4 is the fp32-against-fp64 bound of tests/test_gpu_kernels.py; r is
half a unit in the last place of the tensor's storage type (2^-8 bf16, 2^-11
fp16, 0 for fp32 and for cseq / dh0 / dc0, which are always fp32).

Every case names the kernel it means to run and asserts the planner's answer
(lstm_large_bwd_plan, lstm_large_bwd_persistent, lstm_large_persist_mt), so a
retune cannot silently move it onto another kernel.  The reference itself is
proved against fp64 torch.nn.LSTM / torch.nn.GRU on the CPU
(test_reference_matches_torch_fp64, not marked gpu).

Worst |kernel - ref| / bound measured on an MI355X when this file was written
(hseq / acts / dgates are the 16-bit figures: a correctly rounded bf16 store
alone reaches 2^-8 / (2^-8 + 1e-4) = 0.975; fp32 storage stays below 0.05):

    path (asserted plan: slices, 128x128, pair, persistent)   hseq  cseq  acts  dgates dh0   dc0
    fused step tiles 0-4            (1, 0, 0, no)             0.960 0.014 0.966 0.933 0.003 0.001
    ping-pong fwd, B 300            (2, 0, 0, no)             0.961 0.007 0.966 0.934 0.002 0.001
    ping-pong fwd + fused bwd B 520 (1, 0, 0, no)             0.961 0.010 0.966 0.952 0.002 0.001
    ping-pong GEMM + cell8          (1, 0, 1, no)             0.962 0.011 0.966 0.952 0.004 0.001
    split-K 32x32 x2 / x4 / x8      (2|4|8, 0, 0, no)         0.962 0.068 0.966 0.940 0.008 0.003
    split-K 128x128 x4              (4, 1, 0, no)             0.966 0.083 0.968 0.952 0.017 0.008
    split-K 128x128 x2              (2, 1, 0, no)             0.966 0.121 0.969 0.952 0.025 0.026
    persistent 16-bit, mt 1 / 2     (yes)                     0.965 0.009 0.968 0.952 0.002 0.001
    persistent fp32 backward, H 256 (yes)                     0.017 0.020 0.042 0.001 0.002 0.001
    persistent fp32 backward, H 128 (yes, PDRNN_TUNE rows=0)  0.011 0.014 0.022 0.001 0.001 0.001
    row-owning fp32, H 128          (rows)                    0.011 0.011 0.018 0.002 0.003 0.002

The 238 GPU cases take 4 s together.
"""
import collections

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext

import _large_ref as R
from _tune import set_tune

gpu = pytest.mark.gpu

F64 = torch.float64


# ---------------------------------------------------------------------------
# the reference against torch, fp64, CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("grads", ["all", "final", "seq"])
@pytest.mark.parametrize("ndir,mask,state", [(2, 2, True), (2, 2, False), (1, 1, True), (1, 0, False), (2, 1, True)])
@pytest.mark.parametrize("cell", [0, 1])
def test_reference_matches_torch_fp64(cell, ndir, mask, state, grads):
    """Free-running (its own h fed back, nothing rounded) the reference equals
    fp64 torch.nn.LSTM / nn.GRU to 1e-10 -- outputs, final states, and its
    dgates summed into dW_hh / dx, dh0, dc0 -- with xp / w / wt built from the
    module's parameters by the production packing.  A reversed direction is
    checked against torch on the time-flipped sequence; (2, 1) runs direction
    0 reversed and direction 1 forward against two such modules."""
    torch.manual_seed(10 * cell + ndir + mask)
    H, B, T, I = 5, 3, 4, 6
    lstm = cell == 0
    rev = [bool(mask & (1 << d)) for d in range(ndir)]
    mods = [(torch.nn.LSTM if lstm else torch.nn.GRU)(I, H, 1).double() for _ in range(ndir)]
    x = torch.randn(T, B, I, dtype=F64, requires_grad=True)
    h0 = torch.randn(ndir, B, H, dtype=F64, requires_grad=True) if state else None
    c0 = torch.randn(ndir, B, H, dtype=F64, requires_grad=True) if state and lstm else None
    outs, hns, cns = [], [], []
    for d, m in enumerate(mods):
        xin = x.flip(0) if rev[d] else x
        if lstm:
            o, (hn, cn) = m(xin, (h0[d:d + 1], c0[d:d + 1]) if state else None)
            cns.append(cn[0])
        else:
            o, hn = m(xin, h0[d:d + 1] if state else None)
        outs.append(o.flip(0) if rev[d] else o)
        hns.append(hn[0])
    out, hn = torch.cat(outs, -1), torch.stack(hns)
    cn = torch.stack(cns) if lstm else None
    g = torch.randn_like(out) if grads != "final" else None
    ghn = torch.randn_like(hn) if grads != "seq" else None
    gcn = torch.randn_like(cn) if lstm and grads != "seq" else None
    loss = sum((a * b).sum() for a, b in ((out, g), (hn, ghn), (cn, gcn)) if b is not None)
    loss.backward()

    pack = R.lstm_pack if lstm else R.gru_pack
    with torch.no_grad():
        packs = [pack(m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0, H) for m in mods]
        xp = torch.cat([x @ p[0].t() + p[3] for p in packs], -1)
        w, wt = [p[1] for p in packs], [p[2] for p in packs]
        for d in range(ndir):  # the two layouts of one matrix
            assert torch.equal(R.wt_of(w[d], H), wt[d])
        h0d = h0.detach() if state else None
        c0d = (c0 if lstm else h0).detach() if state else None  # GRU: the fp32 copy of h0
        hseq, cseq, acts = R.forward(xp, w, h0d, c0d, H, mask, cell)
        dgates, dh0, dc0 = R.backward(g, ghn, gcn, wt, cseq, acts, c0d, H, mask, cell)
        # teacher forcing with the reference's own results changes nothing
        for a, b in zip(R.forward(xp, w, h0d, c0d, H, mask, cell, forced=(hseq, cseq)), (hseq, cseq, acts)):
            torch.testing.assert_close(a, b, rtol=0, atol=1e-13)
        for a, b in zip(R.backward(g, ghn, gcn, wt, cseq, acts, c0d, H, mask, cell, forced=dgates), (dgates, dh0, dc0)):
            torch.testing.assert_close(a, b, rtol=0, atol=1e-13)

        tol = dict(rtol=0, atol=1e-10)
        torch.testing.assert_close(hseq, out.detach(), **tol)
        dx = torch.zeros_like(x)
        for d, m in enumerate(mods):
            last = 0 if rev[d] else T - 1
            torch.testing.assert_close(hseq[last, :, d * H:(d + 1) * H], hn[d].detach(), **tol)
            torch.testing.assert_close(cseq[d, last], (cn if lstm else hn)[d].detach(), **tol)
            G = dgates[d]
            dw4 = torch.einsum("tbg,tbh->gh", G, R.h_prev(hseq, h0d, d, H, rev[d]))
            if lstm:
                dwhh, Gx = dw4, G
            else:  # nn.GRU has no n_x block in W_hh and no n_h block in W_ih
                dwhh, Gx = torch.cat([dw4[:2 * H], dw4[3 * H:]], 0), G[..., :3 * H]
            torch.testing.assert_close(dwhh, m.weight_hh_l0.grad, **tol)
            torch.testing.assert_close(torch.einsum("tbg,tbi->gi", Gx, x.detach()), m.weight_ih_l0.grad, **tol)
            dx += Gx @ m.weight_ih_l0
        torch.testing.assert_close(dx, x.grad, **tol)
        if state:
            torch.testing.assert_close(dh0, h0.grad, **tol)
            if lstm:
                torch.testing.assert_close(dc0, c0.grad, **tol)


# ---------------------------------------------------------------------------
# the kernels against the reference
# ---------------------------------------------------------------------------
_DT = {"bf16": (torch.bfloat16, 0, 2.0 ** -8), "fp16": (torch.float16, 1, 2.0 ** -11), "fp32": (torch.float32, 2, 0.0)}
# what a case leaves out: "bare" no h0 / c0 and no dhn / dcn; "final" no dout
# (the motion model's loss: final states only); "strided" dout is a column
# slice of a wider tensor (row stride > width)
VARIANTS = ("full", "bare", "final", "strided")

_worst = collections.defaultdict(float)  # (path, tensor) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nworst |kernel - ref| / bound per path and tensor")
        for (path, name), v in sorted(_worst.items()):
            print(f"RATIO {path:34s} {name:7s} {v:.3f}")


def _inputs(H, B, T, ndir, dt, cell, variant, seed):
    dtype = _DT[dt][0]
    torch.manual_seed(seed)
    dev = "cuda"
    sw = 0.06 if dt == "fp32" else 0.03
    xp = (torch.randn(T, B, ndir * 4 * H, device=dev) * 0.5).to(dtype)
    w = [(torch.randn(4 * H, H, device=dev) * sw).to(dtype) for _ in range(ndir)]
    if cell == 1:
        for t in w:  # the GRU packing: no recurrent term in the n_x slot
            t.view(H, 4, H)[:, 2].zero_()
    wt = [R.wt_of(t, H) for t in w]
    h0 = (torch.randn(ndir, B, H, device=dev) * 0.5).to(dtype)
    c0 = torch.randn(ndir, B, H, device=dev) * 0.5
    wide = (torch.randn(T, B, ndir * H + 64, device=dev) * 0.1).to(dtype)
    dout = wide[:, :, 32:32 + ndir * H]
    if variant != "strided":
        dout = dout.contiguous()
    dhn = torch.randn(ndir, B, H, device=dev) * 0.1
    dcn = torch.randn(ndir, B, H, device=dev) * 0.1 if cell == 0 else None  # (ops/gru_large.py passes none)
    if variant == "bare":
        h0 = c0 = dhn = dcn = None
    if variant == "final":
        dout = None
    return xp, w, wt, h0, c0, dout, dhn, dcn


def _compare(path, dt, cell, got, ref):
    r16 = _DT[dt][2]
    names = ["hseq", "cseq", "acts", "dgates", "dh0", "dc0"]
    rs = [r16, 0.0, r16, r16, 0.0, 0.0]
    bad = []
    for name, r, a, b in zip(names, rs, got, ref):
        if name == "dc0" and cell == 1:
            continue  # the GRU has no cell state: the kernel leaves dc0 unwritten
        assert a.shape == b.shape, name
        a = a.double()
        bound = 2e-5 + (1e-4 + r) * b.abs()
        ratio = float(((a - b).abs() / bound).max()) if bool(torch.isfinite(a).all()) else float("inf")
        _worst[(path, name)] = max(_worst[(path, name)], ratio)
        if not ratio <= 1.0:
            bad.append((name, round(ratio, 3)))
    assert not bad, (path, bad)


def _case(path, H, B, T, ndir, mask, dt, cell, tile, variant):
    """One layer forward + backward on the kernels, each step against fp64."""
    mod = _ext.require()
    args = _inputs(H, B, T, ndir, dt, cell, variant, seed=H + 7 * B + 13 * T + 3 * cell + len(variant))
    xp, w, wt, h0, c0, dout, dhn, dcn = args
    if variant == "strided":
        assert dout.stride(1) > dout.size(2)
    hseq, cseq, acts = mod.lstm_large_fwd(xp, w, h0, c0, H, mask, tile, cell)
    dg, dh0, dc0 = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, H, mask, tile, cell)
    torch.cuda.synchronize()
    ref = R.forward(xp, w, h0, c0, H, mask, cell, forced=(hseq, cseq))
    ref += R.backward(dout, dhn, dcn, wt, cseq, acts, c0, H, mask, cell, forced=dg)
    _compare(path, dt, cell, (hseq, cseq, acts, dg, dh0, dc0), ref)


def _cover(shape_T, dts=("bf16", "fp16")):
    """(dt, variant, T) rows of one shape: every variant and T = 1 in the
    first storage type, the full case in the others."""
    first, rest = dts[0], dts[1:]
    return [(first, v, shape_T) for v in VARIANTS] + [(first, "full", 1)] + [(d, "full", shape_T) for d in rest]


def _plan(mod, B, H, ndir, dt, tile):
    """(splitk, big, pair, persistent backward) as the bindings plan them."""
    code = _DT[dt][1]
    return tuple(mod.lstm_large_bwd_plan(B, H, ndir, code)) + (bool(mod.lstm_large_bwd_persistent(B, H, ndir, code, tile)),)


# --- fused step kernels, tiles 0-4 -----------------------------------------
# H 128: no K split in the backward (4H / 64 = 8 k-tiles is the floor of one
# slice).  B 37 leaves a partial row tile in every tile (32 / 64 / 128 / 256
# rows); B 300 gives tile 3 (256 rows) a full and a partial row block.
@gpu
@pytest.mark.parametrize("dt,variant,T", _cover(3, ("bf16", "fp16", "fp32")))
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cell", [0, 1])
def test_fused_step_every_tile(cell, tile, dt, variant, T):
    mod = _ext.require()
    assert _plan(mod, 37, 128, 2, dt, tile) == (1, 0, 0, False)
    _case(f"fused step tile {tile}", 128, 37, T, 2, 2, dt, cell, tile, variant)


@gpu
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("cell", [0, 1])
def test_fused_step_tile3_two_row_blocks(cell, dt):
    mod = _ext.require()
    assert _plan(mod, 300, 128, 2, dt, 3) == (1, 0, 0, False)
    _case("fused step tile 3", 128, 300, 3, 2, 2, dt, cell, 3, "full")


# --- ping-pong forward step (its backward: 2 slices of 32x32 split-K) --------
@gpu
@pytest.mark.parametrize("dt,variant,T", _cover(3))
@pytest.mark.parametrize("cell", [0, 1])
def test_pingpong_forward_step(monkeypatch, cell, dt, variant, T):
    mod = _ext.require()
    set_tune(monkeypatch, large_pp="2", large_pp_bwd=None, large_tile=None)
    assert _plan(mod, 300, 256, 2, dt, -1) == (2, 0, 0, False)
    _case("pp fwd / split-K 32x32 x2", 256, 300, T, 2, 2, dt, cell, -1, variant)


# --- split-K backward --------------------------------------------------------
# (H, B, ndir, mask, T, forward tile) -> (slices, 128x128).  A forced tile
# keeps H 1024 off the persistent kernels; the backward's split does not
# depend on it.  400 = 3 * 128 + 16 rows.
_SPLITK = {"32x32 x2": ((256, 70, 2, 2, 3, 1), (2, 0)),
           "32x32 x4": ((512, 33, 1, 0, 3, 0), (4, 0)),
           "32x32 x8": ((1024, 16, 1, 1, 3, 0), (8, 0)),
           "128x128 x4": ((1024, 400, 2, 2, 3, 2), (4, 1)),
           "128x128 x2": ((1024, 1000, 2, 2, 2, 3), (2, 1))}


@gpu
@pytest.mark.parametrize("dt,variant,T", _cover(None, ("bf16", "fp16", "fp32")))
@pytest.mark.parametrize("form", list(_SPLITK))
@pytest.mark.parametrize("cell", [0, 1])
def test_splitk_backward(cell, form, dt, variant, T):
    mod = _ext.require()
    (H, B, ndir, mask, Tn, tile), (slices, big) = _SPLITK[form]
    assert _plan(mod, B, H, ndir, dt, tile) == (slices, big, 0, False)
    _case(f"split-K {form}", H, B, T or Tn, ndir, mask, dt, cell, tile, variant)


# --- ping-pong GEMM + cell8 pair, and the fused step at the same shapes ----
@gpu
@pytest.mark.parametrize("pp_bwd,dt,variant,T", [(2,) + row for row in _cover(3)] + [(0, "bf16", "full", 3), (0, "fp16", "full", 3)])
@pytest.mark.parametrize("H,B,ndir,mask", [(512, 520, 1, 0), (256, 520, 2, 2)])
@pytest.mark.parametrize("cell", [0, 1])
def test_pingpong_backward_pair(monkeypatch, cell, H, B, ndir, mask, pp_bwd, dt, variant, T):
    mod = _ext.require()
    set_tune(monkeypatch, large_pp="2", large_pp_bwd=str(pp_bwd), large_tile=None)
    assert _plan(mod, B, H, ndir, dt, -1) == (1, 0, 1 if pp_bwd else 0, False)
    _case("pp GEMM + cell8" if pp_bwd else "pp fwd / fused bwd (B 520)", H, B, T, ndir, mask, dt, cell, -1, variant)


# --- persistent recurrence, 16-bit, H 1024 ---------------------------------
# B 128: one 16-row tile per workgroup (mt 1; two when CUs are reserved for
# RCCL, see below); B 200: two, the last block clamped; B 40 bidirectional
# with direction 1 reversed, always mt 1 with a partial last block.
_P16 = [(128, 1, 0, 1) + row for row in _cover(6)] + [(B, ndir, mask, mt, dt, "full", 6)
                                                      for B, ndir, mask, mt in ((200, 1, 0, 2), (40, 2, 2, 1))
                                                      for dt in ("bf16", "fp16")]


@gpu
@pytest.mark.parametrize("B,ndir,mask,mt,dt,variant,T",  # (ids: the cases keep the names they had beside the removed
                         # tagged-exchange cases, whose last column was 1 where theirs was 0)
                         [pytest.param(*r, id="-".join(map(str, r)) + "-0") for r in _P16])
@pytest.mark.parametrize("cell", [0, 1])
def test_persistent_16bit(cell, B, ndir, mask, mt, dt, variant, T):
    mod = _ext.require()
    H = 1024
    if B == 128 and mod.rccl_cta_reserve() > 0:
        # 8 batch blocks x 32 column blocks fill all 256 CUs: once a communicator
        # in this process has reserved CUs for RCCL, the planner pairs the blocks
        mt = 2
    assert mod.lstm_large_persist_mt(B, H, ndir, _DT[dt][1]) == mt
    assert _plan(mod, B, H, ndir, dt, -1)[3]
    _case(f"persistent 16-bit mt {mt}", H, B, T, ndir, mask, dt, cell, -1, variant)
    mod.persist_check()


# --- row-owning fp32 recurrence, H 128 -------------------------------------
@gpu
@pytest.mark.parametrize("B,T,ndir,mask,variant", [(7, 1, 1, 0, "full"), (40, 3, 2, 2, "full")] +
                         [(200, 3, 1, 0, v) for v in VARIANTS])
@pytest.mark.parametrize("cell", [0, 1])
def test_row_owning_fp32(cell, B, T, ndir, mask, variant):
    mod = _ext.require()
    assert mod.lstm_rows_range_supported(128) and not _plan(mod, B, 128, ndir, "fp32", -1)[3]
    _case("row-owning fp32", 128, B, T, ndir, mask, "fp32", cell, -1, variant)


# --- persistent backward, fp32, H 256 and H 128 (its forward: the per-step
# kernels).  H 128 belongs to the row-owning kernels unless PDRNN_TUNE rows=0.
_P32 = [(256, 7, 1, 1, 4, v) for v in VARIANTS] + [(256, 7, 1, 1, 1, "full"), (256, 300, 2, 2, 3, "full"),
                                                   (128, 7, 1, 1, 4, "full"), (128, 300, 2, 2, 3, "full")]


@gpu
@pytest.mark.parametrize("H,B,ndir,mask,T,variant",  # (the H 256 rows keep the ids they had before H was a column)
                         [pytest.param(*r, id="-".join(map(str, r[1:] if r[0] == 256 else r))) for r in _P32])
@pytest.mark.parametrize("cell", [0, 1])
def test_persistent_fp32_backward(monkeypatch, cell, H, B, ndir, mask, T, variant):
    mod = _ext.require()
    if H == 128:
        set_tune(monkeypatch, rows="0")
    assert mod.lstm_large_persist_mt(B, H, ndir, 2) > 0 and _plan(mod, B, H, ndir, "fp32", -1)[3]
    _case(f"persistent fp32 bwd H {H}", H, B, T, ndir, mask, "fp32", cell, -1, variant)
    mod.persist_check()
