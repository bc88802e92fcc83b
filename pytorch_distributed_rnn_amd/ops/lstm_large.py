"""Large-hidden LSTM stack on the MFMA step kernels (csrc/kernels/lstm_large.hip).

Used when ``H % 64 == 0`` (other H >= 64 are zero-padded up by ops/lstm.py):
16-bit inputs (bf16 / fp16 compute on v_mfma_f32_16x16x32, fp32 master
weights, fp32 cell state and weight gradients) -- the char-LM (H = 1024) and
stacked bidirectional (H = 4096) configurations -- and fp32 inputs (exact fp32
products on v_mfma_f32_16x16x4_f32, e.g. the motion CLI with
``--hidden-units 128``).  Per layer:

* input projection for ALL timesteps and both directions in one library GEMM
  (``Xp = X [W_ih_fwd; W_ih_rev]^T + b``, gate-interleaved columns);
* T launches of the fused recurrent step (MFMA GEMM ``h_{t-1} W_hh^T`` + LSTM
  cell epilogue), both directions per launch;
* backward: one fused first-cell kernel + T launches of the fused BPTT step
  (MFMA ``dgates_t W_hh`` + cell backward of the previous step), then
  ``dW_hh``, ``dW_ih``, ``db`` and ``dX`` as library GEMMs over all
  timesteps with fp32 outputs.

Semantics are torch.nn.LSTM's (gate order i, f, g, o; reference:
src/motion/model.py:9 builds its model on nn.LSTM); parameters stay in the
stock nn.LSTM layout -- the gate interleave is a per-call permutation.

The GRU (ops/gru_large.py) rides on the same kernels and the same host code:
the layer and pipelined-stack Functions, the fp32 weight-gradient helper and
the stack driver here are written once against a ``Cell`` record.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _ext
from ..utils.tune import tune, tune_int
from . import gradsink
from . import shadow as _sh
from .gemm import col_sum, gemm_f32, linear16, mm_kk, mm_nk16


def _tile() -> int:
    """Forced step-kernel tile (PDRNN_TUNE large_tile; -1: the heuristic)."""
    return tune_int("large_tile", -1)


# storage dtype code of the large-H bindings (large_dtype in csrc/bindings.cpp)
_DTYPE_CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def supported(x: Tensor, hidden: int, num_layers: int = 1, bidirectional: bool = False) -> bool:
    """This path covers the shape (LSTM and GRU alike: ops/gru_large.py)."""
    if x.dtype not in _DTYPE_CODE or x.device.type != "cuda" or x.dim() != 3:
        return False
    mod = _ext.native(x.device)
    return mod is not None and hasattr(mod, "lstm_large_fwd") and bool(mod.lstm_large_supported(hidden))


def _bwd_persistent(mod, B: int, H: int, ndir: int, cdt: torch.dtype, tile: int) -> bool:
    """lstm_large_bwd would run this shape as one grid-synced persistent launch
    (an extension without the query: assume so, i.e. never overlap it)."""
    query = getattr(mod, "lstm_large_bwd_persistent", None)
    return True if query is None else bool(query(B, H, ndir, _DTYPE_CODE[cdt], tile))


def shadow(w: Tensor, kind: str, cdt: torch.dtype, hidden: int) -> Tensor:
    """Compute-dtype copy of an fp32 master weight in the layout a kernel reads.

    The copy is 16-bit, or fp32 on the fp32 path. It is cached on the parameter
    and rebuilt only when the master changed: the version counter moves on every
    in-place update, and FusedAdam's native step bumps it explicitly. After an
    optimizer step, the first stale lookup rebuilds every stale shadow of the
    device in one pack launch (ops/shadow.py, kernels/shadow_pack.hip).

    kind: "i" gate-interleaved rows (forward step GEMM / input projection),
          "p" stored layout (dX GEMM), "t" transposed [I, 4H] (BPTT step GEMM)."""
    if kind == "p" and w.dtype == cdt:
        return w.detach()  # the master itself
    if kind not in ("i", "p", "t"):
        raise ValueError(kind)
    rows, cols = w.shape
    box = []  # the output buffer, for the builder (which must not hold the master)

    def alloc():
        box.append(torch.empty((cols, rows) if kind == "t" else (rows, cols), device=w.device, dtype=cdt))
        return box[0]

    def build(src):
        t = box[0]
        if kind == "i":
            return [_interleave_job(t, src, hidden)]
        if kind == "p":
            return [_sh.job(t, src)]
        return [_sh.job(t, src.t())]

    return _sh.get(w, (kind, cdt), [w], alloc, build)


def _interleave_job(dst: Tensor, src: Tensor, hidden: int):
    """dst[4u + q] = src[q*H + u]: gate-blocked -> gate-interleaved rows."""
    k = src.shape[1]
    return _sh.job(dst.view(hidden, 4, k), src.view(4, hidden, k).transpose(0, 1))


def _shadow_cat(ws: List[Tensor], cdt: torch.dtype, hidden: int) -> Tensor:
    """Both directions' interleaved input weights stacked [ndir*4H, I] (one
    input-projection GEMM for both), cached on the first weight."""
    if len(ws) == 1:
        return shadow(ws[0], "i", cdt, hidden)
    n4 = 4 * hidden
    key = ("icat", cdt, tuple(id(w) for w in ws))
    box = []

    def alloc():
        box.append(torch.empty(len(ws) * n4, ws[0].shape[1], device=ws[0].device, dtype=cdt))
        return box[0]

    def build(*srcs):
        t = box[0]
        return [_interleave_job(t[d * n4:(d + 1) * n4], src, hidden) for d, src in enumerate(srcs)]

    return _sh.get(ws[0], key, list(ws), alloc, build)


def _bias_cat(weights, ndir: int, hidden: int, device) -> Tensor:
    """b_ih + b_hh of every direction, gate-interleaved and concatenated (the
    projection GEMM's fp32 epilogue bias), cached like the shadow weights and
    rebuilt only after the biases change."""
    bs = [weights[4 * d + k] for d in range(ndir) for k in (2, 3)]
    n4 = 4 * hidden
    box = []

    def alloc():
        box.append(torch.zeros(ndir * n4, device=device, dtype=torch.float32))
        return box[0]

    def build(*srcs):
        t = box[0]
        jobs = []
        for d in range(ndir):
            b = t[d * n4:(d + 1) * n4].view(hidden, 4)  # interleaved: [u][q] = row q*H + u
            pair = [src.view(4, hidden).t() for src in srcs[2 * d:2 * d + 2] if src is not None]
            if len(pair) == 2:
                jobs.append(_sh.job(b, pair[0], pair[1]))
            elif pair:
                jobs.append(_sh.job(b, pair[0]))
            # no bias at all: the buffer stays zero
        return jobs

    return _sh.get(weights[0], ("bias", ndir, hidden), bs, alloc, build)


class Cell(NamedTuple):
    """What differs between the cells on this path; the layer, the pipelined
    stack, the weight-gradient helper and the stack driver below are written
    once against it (LSTM here, GRU in ops/gru_large.py).  Both cells ride on
    the step kernels' four-column quad, so dgates is [.., 4H] for either;
    column and row positions below are in units of H."""
    cell: int            # id the bindings take (csrc/include/pdrnn/api.h: PdrnnLstmLargeStepArgs.cell)
    gates: int           # gate rows of the parameters: W_ih [gates*H, I], W_hh [gates*H, H]
    has_c: bool          # a cell state of its own (c0 / cseq / dcn / dc0); else the fp32 h rides in that slot
    xcols: int           # dgates[:, :xcols*H] is the x side (dW_ih, dX)
    hh_blocks: Tuple[Tuple[int, int, int], ...]  # (c0, c1, r0): dgates columns [c0, c1) -> dW_hh rows from r0
    # db_ih is the row sums rs of the dW_ih pass; db_hh is the same tensor
    # (None) or db_hh(rs, G [T*B, 4H], H, out) fills ``out`` [gates*H]
    db_hh: Optional[Callable]
    # shadows(weights, ndir, H, I, cdt, device) -> (projection stack [ndir*4H, I]
    # gate-interleaved, folded fp32 bias [ndir*4H], and per direction the
    # interleaved W_hh (forward step), W_ih as stored (dX) and W_hh^T (BPTT))
    shadows: Callable
    # 16-bit layers: backward16(ctx, dgates, dh0, dc0, hseq, h0c, x2, wih) ->
    # the layer Function's gradients (the one place the cells' structure differs)
    backward16: Callable


def _lstm_shadows(weights, ndir: int, H: int, I: int, cdt, device):
    w_ih = [weights[4 * d] for d in range(ndir)]
    w_hh = [weights[4 * d + 1] for d in range(ndir)]
    return (_shadow_cat(w_ih, cdt, H), _bias_cat(weights, ndir, H, device), [shadow(w, "i", cdt, H) for w in w_hh],
            [shadow(w, "p", cdt, H) for w in w_ih], [shadow(w, "t", cdt, H) for w in w_hh])


# ---------------------------------------------------------------------------
# Cross-layer overlap in the fp32 backward: layer l's recurrence (90 of 256
# CUs at the motion batch) needs only the layer above's dX, not its weight
# gradients.  The layer above records an event right after its dX GEMM and
# hangs it on the dX tensor; this layer's recurrence then runs on a
# high-priority side stream that waits for that event only, while the main
# stream is still busy with the layer above's dW GEMMs.  The main stream
# joins the side stream before this layer's own GEMMs (and every gradient is
# still returned through autograd on the main stream: DDP hooks unchanged).
_SIDE = {}


def _side_stream(device) -> "torch.cuda.Stream":
    s = _SIDE.get(device)
    if s is None:
        s = _SIDE[device] = torch.cuda.Stream(device=device, priority=-1)
    return s


def overlap_on() -> bool:
    return tune("large_overlap", "1") != "0"


def run_recurrence(dhseq: Optional[Tensor], fn, inputs: Sequence[Optional[Tensor]], persistent: bool = False):
    """fn() -> tensors: the layer's backward recurrence, on the side stream
    when the upstream gradient carries a ready event (see above), inline
    otherwise.  ``inputs``: the tensors fn reads, as autograd delivered them;
    fn converts them itself, so any conversion kernel runs on the side stream
    after the event.  The event covers the main stream up to the dX GEMM
    only, so the layer's Function must not let autograd materialise zero
    gradients (``ctx.set_materialize_grads(False)``): such a zero fill is
    queued on the main stream after the event, and the side stream read it
    before it ran (uninitialised dc carry: wrong gradients one run in a few,
    tools/pipe_determinism.py).  ``persistent``: the recurrence is one
    grid-synced persistent launch, whose co-residency is checked against an
    idle device only -- it runs inline, never beside the side-stream GEMMs."""
    if persistent:
        return fn()
    ev = getattr(dhseq, "_pdrnn_ready", None) if dhseq is not None else None
    if ev is not None and getattr(dhseq, "_pdrnn_ready_version", None) != dhseq._version:
        ev = None  # written after the event (e.g. an in-place gradient accumulation)
    if ev is None or not overlap_on():
        return fn()
    main = torch.cuda.current_stream(dhseq.device)
    side = _side_stream(dhseq.device)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        out = fn()
    for t in inputs:  # main-stream tensors read on the side stream
        if t is not None:
            t.record_stream(side)
    for t in out:  # side-stream tensors read on the main stream
        if t is not None:
            t.record_stream(main)
    main.wait_stream(side)
    return out


def mark_ready(dx: Optional[Tensor]) -> Optional[Tensor]:
    """Record the event the layer below waits for (after this layer's dX)."""
    if dx is not None and dx.is_cuda and overlap_on():
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dx.device))
        dx._pdrnn_ready = ev
        dx._pdrnn_ready_version = dx._version
    return dx


def _final_states(cell: Cell, hs: Sequence[Tensor], cs: Sequence[Tensor], cdt) -> Tuple[Tensor, Optional[Tensor]]:
    """The [B, H] final hidden states ``hs`` (one per direction or layer)
    gathered into a fresh [n, B, H] tensor, and for a cell with a c state the
    fp32 ``cs`` likewise, in the compute dtype.  The LSTM's two gathers are one
    pack launch (ops/shadow.py); the GRU's is a copy per entry, as it always
    was -- moving it onto the pack launch changes its launch sequence, which is
    a change of its own."""
    hn = hs[0].new_empty(len(hs), *hs[0].shape)
    if not cell.has_c:
        for k, h in enumerate(hs):
            hn[k].copy_(h)
        return hn, None
    cn = cs[0].new_empty(len(cs), *cs[0].shape, dtype=cdt)
    _sh.pack([_sh.job(hn[k], h) for k, h in enumerate(hs)] + [_sh.job(cn[k], c) for k, c in enumerate(cs)], hn.device)
    return hn, cn


class _StackStates(torch.autograd.Function):
    """Per-layer final h and c ([ndir, B, H] each) stacked into nn.LSTM's
    [layers*ndir, B, H] pair by one pack launch (ops/shadow.py) instead of a
    slice copy per layer and state; the backward hands each layer its slices."""

    @staticmethod
    def forward(ctx, L, *states):
        ctx.set_materialize_grads(False)
        outs, jobs, ns = [], [], []
        for group in (states[:L], states[L:]):
            n = group[0].shape[0]
            out = group[0].new_empty(n * L, *group[0].shape[1:])
            jobs += [_sh.job(out[l * n:(l + 1) * n], s) for l, s in enumerate(group)]
            outs.append(out)
            ns.append(n)
        _sh.pack(jobs, states[0].device)
        ctx.L, ctx.ns = L, ns
        return tuple(outs)

    @staticmethod
    def backward(ctx, dh, dc):
        L = ctx.L
        grads = []
        for g, n in zip((dh, dc), ctx.ns):
            grads += [g[l * n:(l + 1) * n] if g is not None else None for l in range(L)]
        return (None, *grads)


def stack_layers(states: List[Tensor]) -> Tensor:
    """Per-layer [ndir, B, H] states -> [layers*ndir, B, H] (slice copies,
    autograd-tracked; a single layer is returned as is)."""
    if len(states) == 1:
        return states[0]
    n = states[0].shape[0]
    out = states[0].new_empty(n * len(states), *states[0].shape[1:])
    for l, s in enumerate(states):
        out[l * n:(l + 1) * n] = s
    return out


def _cols(t: Tensor, c0: int, c1: int) -> Tensor:
    """Columns [c0, c1) of a 2-D tensor: the tensor itself when that is all of
    them (a view costs host time, and this path is bound by it)."""
    return t if c0 == 0 and c1 == t.shape[1] else t[:, c0:c1]


def _weight_grads(cell: Cell, G3: Tensor, hd: Tensor, h0: Optional[Tensor], xin: Tensor, d: int, t0: int, t1: int,
                  dwih: Optional[Tensor] = None, dwhh: Optional[Tensor] = None, accumulate: bool = False,
                  pad: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """Steps [t0, t1) of one direction's fp32 weight gradients, every product
    on the fp32-product MFMA GEMM (kernels/gemm_f32.hip) -> (dW_ih, dW_hh, rs).

    G3 [T, B, 4H]: the direction's dgates; hd [T, B, H]: its output sequence
    (a strided view of hseq will do: no h_prev copy); h0 [B, H] or None;
    xin [T, B, I]: the layer input.  dW_hh = sum_t dgates_t^T h_prev(t), block
    by block of ``cell.hh_blocks``: h_prev(t) is h_{t-1} forward (d = 0) and
    h_{t+1} reverse (d = 1), and the step next to the initial state pairs with
    h0 as a second K segment.  dW_ih = dgates^T x over the x-side columns, with
    rs, the row sums of that pass (the bias gradient), alongside.  ``dwih`` /
    ``dwhh``: written in place (``accumulate``: added to; rs never is), fresh
    tensors otherwise.  ``pad``: a narrow input goes through padded_cols
    (needs ``dwih``)."""
    T, B, H4 = G3.shape
    H = H4 // 4
    G = G3.view(T * B, H4)
    if d == 0:
        lo, hi, shift, edge, at_edge = max(t0, 1), t1, -1, 0, t0 == 0
    else:
        lo, hi, shift, edge, at_edge = t0, min(t1, T - 1), 1, T - 1, t1 == T
    if dwhh is None:
        dwhh = G3.new_empty(cell.gates * H, H)
    if hi > lo:
        Gs, hs = G[lo * B:hi * B], hd[lo + shift:hi + shift].reshape(-1, H)
    g0 = G[edge * B:(edge + 1) * B] if at_edge and h0 is not None else None
    for c0, c1, r0 in cell.hh_blocks:
        out = dwhh if c1 - c0 == cell.gates else dwhh[r0 * H:(r0 + c1 - c0) * H]
        seg = (_cols(g0, c0 * H, c1 * H), h0) if g0 is not None else None
        if hi > lo:
            gemm_f32(_cols(Gs, c0 * H, c1 * H), True, hs, True, pairs2=seg, out=out, accumulate=accumulate)
        elif seg is not None:
            gemm_f32(seg[0], True, seg[1], True, out=out, accumulate=accumulate)
        elif not accumulate:
            out.zero_()
    x2 = xin.reshape(T * B, xin.shape[2])
    Gx = _cols(G, 0, cell.xcols * H)
    if t1 - t0 < T:
        Gx, x2 = Gx[t0 * B:t1 * B], x2[t0 * B:t1 * B]
    if pad and x2.shape[1] % 32:  # narrow input (motion: 9 features): whole, aligned column tiles
        c, rs = gemm_f32(Gx, True, padded_cols(x2), True, rowsum=True)
        dwih.add_(c[:, :x2.shape[1]]) if accumulate else dwih.copy_(c[:, :x2.shape[1]])
    else:
        dwih, rs = gemm_f32(Gx, True, x2, True, rowsum=True, out=dwih, accumulate=accumulate)
    return dwih, dwhh, rs


def _state_grads(ctx, dh0, dc0, h0_dtype, c0_dtype) -> List[Optional[Tensor]]:
    """[dh0, dc0] for autograd: cast to the dtype the initial state came in
    (a list of per-layer [B, H] is stacked first); None for a state that was
    not given or needs no gradient (a detached carried state -- truncated
    BPTT -- costs no stack or cast kernel)."""
    out: List[Optional[Tensor]] = []
    for k, (g, dtype) in enumerate(((dh0, h0_dtype), (dc0, c0_dtype)), 1):
        if g is None or dtype is None or not ctx.needs_input_grad[k]:
            out.append(None)
        else:
            out.append((torch.stack(g) if isinstance(g, list) else g).to(dtype))
    return out


class _LargeLayer(torch.autograd.Function):
    """One layer of either cell, 1 or 2 directions.  x: [T, B, I] (compute
    dtype); cfg: (cell, hidden, ndir, tile); weights: per direction (w_ih,
    w_hh, b_ih, b_hh), fp32 master parameters (biases may be None).  Returns
    (hseq, hn, cn), cn None for a cell without a c state."""

    @staticmethod
    def forward(ctx, x, h0, c0, cfg, *weights):
        # unused outputs come back as None, not as a zero fill queued on the
        # main stream after the ready event (run_recurrence)
        ctx.set_materialize_grads(False)
        cell, H, ndir, tile = cfg
        cdt = x.dtype
        T, B, I = x.shape
        mod = _ext.native(x.device)
        # forward in gate-interleaved order; backward in torch's gate-blocked
        # order: W_ih as stored (dX GEMM), W_hh transposed (BPTT step GEMM)
        proj, bias, whh_i, wih_p, wt = cell.shadows(weights, ndir, H, I, cdt, x.device)
        if cdt == torch.float32:  # fp32-product MFMA GEMM (kernels/gemm_f32.hip), fp32 bias in the epilogue
            xp = gemm_f32(x.reshape(T * B, I), False, proj, False, bias=bias)[0]
        else:  # in-tree MFMA GEMM, fp32 bias added before the 16-bit rounding (ops/gemm.py)
            xp = linear16(x.reshape(T * B, I), proj, bias)
        xp = xp.view(T, B, ndir * 4 * H)
        h0c = h0.to(cdt).contiguous() if h0 is not None else None
        s0 = c0 if cell.has_c else h0  # the fp32 state beside h: c, or the GRU's own h
        s0 = s0.float().contiguous() if s0 is not None else None
        rev_mask = 2 if ndir == 2 else 0
        hseq, sseq, acts = mod.lstm_large_fwd(xp, whh_i, h0c, s0, H, rev_mask, tile, cell.cell)
        last = [T - 1, 0][:ndir]
        hn, cn = _final_states(cell, [hseq[last[d], :, d * H:(d + 1) * H] for d in range(ndir)],
                               [sseq[d, last[d]] for d in range(ndir)] if cell.has_c else (), cdt)
        ctx.save_for_backward(x, hseq, sseq, acts, h0c, s0, *wih_p, *wt)
        ctx.cfg = (cell, H, ndir, tile, rev_mask, [w is not None for w in weights],
                   h0.dtype if h0 is not None else None, c0.dtype if cell.has_c and c0 is not None else None)
        ctx.params = weights  # (gradsink: the LSTM's 16-bit backward may accumulate into their .grad)
        ctx.direct = gradsink.enabled()
        return hseq, hn, cn

    @staticmethod
    def backward(ctx, dhseq, dhn, dcn):
        cell, H, ndir, tile, rev_mask, has_w, h0_dtype, c0_dtype = ctx.cfg
        x, hseq, sseq, acts, h0c, s0, *ws = ctx.saved_tensors
        wih, wt = ws[:ndir], list(ws[ndir:])                        # wt: [H, 4H], gate-blocked
        cdt = x.dtype
        T, B, I = x.shape
        mod = _ext.native(x.device)

        def bptt():
            dout = dhseq.to(cdt).contiguous() if dhseq is not None else None
            dhn_f = dhn.float().contiguous() if dhn is not None else None
            dcn_f = dcn.float().contiguous() if dcn is not None else None
            return mod.lstm_large_bwd(dout, dhn_f, dcn_f, wt, sseq, acts, s0, H, rev_mask, tile, cell.cell)

        dgates, dh0, dc0 = run_recurrence(dhseq, bptt, [dhseq, dhn, dcn, sseq, acts, s0, *wt],
                                          _bwd_persistent(mod, B, H, ndir, cdt, tile))
        if cdt != torch.float32:
            return cell.backward16(ctx, dgates, dh0, dc0, hseq, h0c, x.reshape(T * B, I), wih)
        # fp32 layers.  dX of both directions in one launch (K segments) and
        # first, so the layer below can start its recurrence beside this
        # layer's dW GEMMs (run_recurrence); it is returned as the very tensor
        # mark_ready tagged: a view would drop the ready event
        dx = None
        G3 = [dgates[d] for d in range(ndir)]
        G = [g.view(T * B, 4 * H) for g in G3]
        if ctx.needs_input_grad[0]:
            Gx = [_cols(g, 0, cell.xcols * H) for g in G]
            dx = gemm_f32(Gx[0], False, wih[0], True, pairs2=(Gx[1], wih[1]) if ndir > 1 else None)[0]
            dx = mark_ready(dx.view(T, B, I))
        grads: List[Optional[Tensor]] = []
        for d in range(ndir):
            dwih, dwhh, dbih = _weight_grads(cell, G3[d], hseq[:, :, d * H:(d + 1) * H],
                                             h0c[d] if h0c is not None else None, x, d, 0, T)
            dbhh = dbih
            if cell.db_hh is not None:
                dbhh = cell.db_hh(dbih, G[d], H, dbih.new_empty(cell.gates * H))
            grads += [dwih, dwhh, dbih if has_w[4 * d + 2] else None, dbhh if has_w[4 * d + 3] else None]
        return (dx, *_state_grads(ctx, dh0, dc0 if cell.has_c else None, h0_dtype, c0_dtype), None, *grads)


def _backward_gemms16(ctx, dgates, dh0, dc0, hseq, h0c, x2, wih):
    """16-bit layers: weight and input gradients on the in-tree MFMA GEMM
    (ops/gemm.py): dW_hh = sum_t dgates_t^T h_prev(t) with the initial-state
    pairing folded in as a second K segment, dW_ih = dG^T X, dX of both
    directions in one launch (K segments), fp32 accumulation throughout.

    The GRU's 16-bit backward (ops/gru_large.py:_backward_gemms16) is built
    differently -- an h_prev concatenation instead of K-segment pairs, and no
    gradsink; moving it onto this function changes its launches and speed, so
    that is a change of its own."""
    cell, H, ndir, tile, rev_mask, has_w, h0_dtype, c0_dtype = ctx.cfg
    T, B, I = ctx.saved_tensors[0].shape
    grads: List[Optional[Tensor]] = []
    Gs = []
    params = getattr(ctx, "params", None)
    for d in range(ndir):
        G = dgates[d].view(T * B, 4 * H)                         # gate-blocked = parameter order
        Gs.append(G)
        hd = hseq[:, :, d * H:(d + 1) * H]                       # strided view, row stride ndir*H
        pairs = []
        if T > 1:
            if d == 0:
                pairs.append((G[B:], hd[:-1].reshape((T - 1) * B, H)))
            else:
                pairs.append((G[:(T - 1) * B], hd[1:].reshape((T - 1) * B, H)))
        if h0c is not None:
            pairs.append((G[:B] if d == 0 else G[(T - 1) * B:], h0c[d]))
        # direct mode (ops/gradsink.py): this direction's weight and bias
        # gradients accumulated into the flat gradient views by the GEMM
        # epilogue / split-K sum and the column-sum pass -- nothing for
        # autograd to add
        pw = params[4 * d:4 * d + 4] if params is not None else (None,) * 4
        sinks = [gradsink.sink(w, ctx.direct) if w is not None else None for w in pw]
        if params is not None and pairs and all(sk is not None for sk, w in zip(sinks, pw) if w is not None) and \
                sinks[0] is not None and sinks[1] is not None:
            mm_kk(pairs, accumulate_into=sinks[1])
            mm_kk([(G, x2)], accumulate_into=sinks[0])
            bs = [sk for sk in sinks[2:] if sk is not None]
            if bs:
                col_sum(G, accumulate_into=bs)
            grads += [None, None, None, None]
            continue
        dwhh = mm_kk(pairs) if pairs else torch.zeros(4 * H, H, device=G.device, dtype=torch.float32)
        dwih = mm_kk([(G, x2)])
        db = col_sum(G)  # in-tree deterministic column sums (fp32 accumulation of the 16-bit G)
        grads += [dwih, dwhh, db if has_w[4 * d + 2] else None, db if has_w[4 * d + 3] else None]
    dx = mm_nk16([(Gs[d], wih[d]) for d in range(ndir)]).view(T, B, I) if ctx.needs_input_grad[0] else None
    return (dx, *_state_grads(ctx, dh0, dc0, h0_dtype, c0_dtype), None, *grads)


# ---------------------------------------------------------------------------
# Stacked-layer pipeline (fp32, one direction, H = 128 on the row-owning
# kernels).  The sequence is cut into C time chunks and every layer runs on a
# stream of its own (layer 0 on the caller's): layer l + 1 computes chunk c --
# its input projection, then its recurrence -- while layer l computes chunk
# c + 1, so the layers' recurrences (90 of 256 CUs each at the motion batch)
# overlap instead of running one after the other.  The backward is the mirror
# image: layer l's BPTT of chunk c starts as soon as the layer above has
# produced dX for that chunk, and each layer's weight gradients follow its
# recurrence on its stream (beside the recurrences of the layers below).
# Chunk boundaries carry the state through the full-length tensors
# (lstm_rows_fwd_range / lstm_rows_bwd_range), so the forward is
# bit-identical to one whole-sequence launch per layer.
#
# One stream per layer, nothing more: with GPU_MAX_HW_QUEUES = 4 (HIP's
# default) further streams share hardware queues, and an event wait on one of
# them stalls the others (measured: separate projection and weight-gradient
# streams made the step 25-70 % slower, profiles/r4/pipe/).
_PIPE_STREAMS = {}


def _pipe_stream(device, l: int) -> "torch.cuda.Stream":
    if l == 0:
        return torch.cuda.current_stream(device)
    s = _PIPE_STREAMS.get((device, l))
    if s is None:
        s = _PIPE_STREAMS[(device, l)] = torch.cuda.Stream(device=device, priority=-1)
    return s


def pipeline_chunks(T: int) -> List[Tuple[int, int]]:
    """[t0, t1) time chunks of the stacked-layer pipeline (PDRNN_TUNE large_chunks,
    default 3: at T = 128 4.54-4.57 ms/step against 4.69-4.79 with 2, 4 or 5
    chunks and 4.92 with 6, profiles/r4/pipe/p6_*)."""
    c = max(1, min(tune_int("large_chunks", 3), T))
    return [(T * i // c, T * (i + 1) // c) for i in range(c)]


def pipeline_ok(x: Tensor, hidden: int, num_layers: int, bidirectional: bool, dropout: float,
                training: bool) -> bool:
    """The stacked-layer pipeline covers unidirectional fp32 stacks of >= 2
    layers at the row-owning kernels' H (PDRNN_TUNE large_pipe=0 turns it off)."""
    if tune("large_pipe", "1") == "0" or _tile() >= 0:
        return False
    if x.dtype != torch.float32 or not x.is_cuda or bidirectional or num_layers < 2 or (dropout > 0 and training):
        return False
    mod = _ext.native(x.device)
    return mod is not None and hasattr(mod, "lstm_rows_range_supported") and bool(mod.lstm_rows_range_supported(hidden))


def _event(stream) -> "torch.cuda.Event":
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def pipeline_streams(device, L: int) -> List["torch.cuda.Stream"]:
    """One stream per layer (layer 0: the caller's); the side streams first
    wait for everything the caller has queued (weights, shadows, buffers)."""
    main = torch.cuda.current_stream(device)
    streams = [_pipe_stream(device, l) for l in range(L)]
    for s in streams[1:]:
        s.wait_stream(main)
    return streams


def pipeline_join(streams) -> None:
    main = streams[0]
    for s in streams[1:]:
        main.wait_stream(s)


def pipeline_forward(streams, chunks, project, recur) -> None:
    """Issue the stacked-layer forward: for every chunk and layer,
    ``project(l, t0, t1)`` (l > 0, once the layer below has finished the
    chunk) then ``recur(l, t0, t1)``, on layer l's stream."""
    L = len(streams)
    done = [[None] * len(chunks) for _ in range(L)]
    for ci, (t0, t1) in enumerate(chunks):
        for l in range(L):
            with torch.cuda.stream(streams[l]):
                if l > 0:
                    streams[l].wait_event(done[l - 1][ci])
                    project(l, t0, t1)
                recur(l, t0, t1)
                done[l][ci] = _event(streams[l])


def pipeline_backward(streams, chunks, project, recur, finish) -> None:
    """Issue the stacked-layer backward, last chunk first: ``project(l, t0,
    t1)`` (dX of layer l + 1 for the chunk, once that layer has finished it),
    ``recur(l, first, t0, t1)`` (first: the chunk that starts the layer's
    BPTT), and after a layer's last chunk ``finish(l)`` (its weight
    gradients), on layer l's stream."""
    L = len(streams)
    done = [[None] * len(chunks) for _ in range(L)]
    last = len(chunks) - 1
    for ci in range(last, -1, -1):
        t0, t1 = chunks[ci]
        for l in range(L - 1, -1, -1):
            with torch.cuda.stream(streams[l]):
                if l < L - 1:
                    streams[l].wait_event(done[l + 1][ci])
                    project(l, t0, t1)
                recur(l, ci == last, t0, t1)
                done[l][ci] = _event(streams[l])
                if ci == 0:
                    finish(l)


def _add_bias_sinks(rs: Tensor, bi: Optional[Tensor], bh: Optional[Tensor]) -> None:
    """Direct mode (ops/gradsink.py): the row sums added into the flat
    gradient views of b_ih and b_hh as they come out of the dW_ih pass."""
    # (same storage too: two separately allocated gradients can sit side by
    # side in the caching allocator)
    if bi is not None and bh is not None and bh.data_ptr() == bi.data_ptr() + bi.numel() * 4 and \
            bi.untyped_storage().data_ptr() == bh.untyped_storage().data_ptr():
        # b_ih, b_hh adjacent in the flat gradient: one launch for both
        torch.as_strided(bi, (2, bi.numel()), (bi.numel(), 1)).add_(rs)
        return
    for bg in (bi, bh):
        if bg is not None:
            bg.add_(rs)


class _PipelinedStack(torch.autograd.Function):
    """All layers of a unidirectional fp32 stack of either cell,
    chunk-pipelined (see above).  x: [T, B, I] fp32; h0 / c0: [L, B, H] or None;
    cfg: (cell, hidden, layers, per, chunks); weights: nn.LSTM / nn.GRU
    ``_all_weights`` order, ``per`` (2 or 4) tensors per layer.  Returns
    (hseq of the last layer, hn, cn), cn None for a cell without a c state."""

    @staticmethod
    def forward(ctx, x, h0, c0, cfg, *weights):
        ctx.set_materialize_grads(False)
        cell, H, L, per, chunks = cfg
        T, B, I = x.shape
        dev = x.device
        lw = [list(weights[l * per:(l + 1) * per]) + ([None, None] if per == 2 else []) for l in range(L)]
        # per layer: projection stack [4H, I_l], folded bias, then one-entry
        # lists of the interleaved W_hh, W_ih as stored and W_hh^T
        proj, bias, whh_i, wih_p, wt = zip(*[cell.shadows(lw[l], 1, H, I if l == 0 else H, torch.float32, dev)
                                             for l in range(L)])
        h0s = [h0[l].float().contiguous() if h0 is not None else None for l in range(L)]
        # the fp32 state beside h: c, or the GRU's own h (the same tensors)
        s0s = [c0[l].float().contiguous() if c0 is not None else None for l in range(L)] if cell.has_c else h0s
        hseq = [x.new_empty(T, B, H) for _ in range(L)]
        sseq = [x.new_empty(T, B, H) for _ in range(L)]
        acts = [x.new_empty(T, B, 4 * H) for _ in range(L)]
        xps = [gemm_f32(x.reshape(T * B, I), False, proj[0], False, bias=bias[0])[0].view(T, B, 4 * H)]
        xps += [x.new_empty(T, B, 4 * H) for _ in range(1, L)]
        rec = pipeline_streams(dev, L)
        fwd_range, cid = _ext.native(dev).lstm_rows_fwd_range, cell.cell

        def project(l, t0, t1):  # this chunk's input projection
            gemm_f32(hseq[l - 1][t0:t1].view(-1, H), False, proj[l], False, bias=bias[l],
                     out=xps[l][t0:t1].view(-1, 4 * H))

        def recur(l, t0, t1):
            fwd_range(xps[l][t0:t1], whh_i[l][0], h0s[l], s0s[l], hseq[l], sseq[l], acts[l], t0, t1, cid)

        pipeline_forward(rec, chunks, project, recur)
        pipeline_join(rec)
        hn, cn = _final_states(cell, [hq[T - 1] for hq in hseq], [sq[T - 1] for sq in sseq] if cell.has_c else (),
                               torch.float32)
        ctx.save_for_backward(x, *hseq, *sseq, *acts, *[w[0] for w in wih_p], *[w[0] for w in wt])
        ctx.states = (h0s, s0s)
        # (gradsink, LSTM only: the backward may accumulate into the parameters' .grad itself)
        ctx.params = lw if cell.has_c else None
        ctx.direct = gradsink.enabled()
        ctx.cfg = (cell, H, L, per, chunks, [[w is not None for w in ws] for ws in lw],
                   h0.dtype if h0 is not None else None, c0.dtype if cell.has_c and c0 is not None else None)
        return hseq[L - 1], hn, cn

    @staticmethod
    def backward(ctx, dhseq, dhn, dcn):
        cell, H, L, per, chunks, has_w, h0_dtype, c0_dtype = ctx.cfg
        h0s, s0s = ctx.states
        sv = ctx.saved_tensors
        x = sv[0]
        hseq, sseq, acts, wp, wt = (sv[1 + k * L:1 + (k + 1) * L] for k in range(5))
        T, B, I = x.shape
        dev = x.device
        R, xc = cell.gates * H, cell.xcols * H
        dgates = [x.new_empty(T, B, 4 * H) for _ in range(L)]
        douts = [x.new_empty(T, B, H) for _ in range(L - 1)]
        douts.append(dhseq.float().contiguous() if dhseq is not None else None)
        dhb = [x.new_empty(B, H) for _ in range(L)]  # gradients leaving a chunk's first step
        dcb = [x.new_empty(B, H) for _ in range(L)]  # (the kernel's dc0 slot; a cell without a c state leaves it unused)
        carry = [x.new_empty(B, H) for _ in range(L)]
        dhn_l = [dhn[l].float().contiguous() if dhn is not None else None for l in range(L)]
        dcn_l = [dcn[l].float().contiguous() if dcn is not None else None for l in range(L)]
        ins = [x] + list(hseq[:-1])  # each layer's input sequence
        # direct mode (ops/gradsink.py): a layer whose w_ih / w_hh (and biases)
        # all have flat .grad views accumulates into them in the GEMM epilogue
        direct = [False] * L
        if ctx.params is not None:
            sinks = [[gradsink.sink(w, ctx.direct) for w in ws] for ws in ctx.params]
            direct = [all(sk is not None for sk, w in zip(sinks[l], ctx.params[l]) if w is not None) for l in range(L)]
        dwih = [sinks[l][0] if direct[l] else x.new_empty(R, t.shape[2]) for l, t in enumerate(ins)]
        dwhh = [sinks[l][1] if direct[l] else x.new_empty(R, H) for l in range(L)]
        dbih = [x.new_empty(R) for _ in range(L)]
        dbhh = [x.new_empty(R) for _ in range(L)] if cell.db_hh is not None else dbih
        rec = pipeline_streams(dev, L)
        bwd_range, cid, has_c = _ext.native(dev).lstm_rows_bwd_range, cell.cell, cell.has_c

        def project(l, t0, t1):  # this chunk's dout = dX of the layer above
            # (one K slice: split-K partials and their sum beside the
            # recurrences cost more than they recover, profiles/r4/pipe/p6_*)
            gemm_f32(_cols(dgates[l + 1][t0:t1].view(-1, 4 * H), 0, xc), False, wp[l + 1], True,
                     out=douts[l][t0:t1].view(-1, H), splitk=1)

        def recur(l, first, t0, t1):
            dout = douts[l][t0:t1] if douts[l] is not None else None
            dc_in = (dcn_l[l] if first else dcb[l]) if has_c else None
            bwd_range(dout, dhn_l[l] if first else dhb[l], dc_in, wt[l], sseq[l], acts[l], s0s[l], dgates[l], dhb[l],
                      dcb[l], carry[l], t0, t1, cid)

        def finish(l):  # the layer's recurrence is done: its weight gradients, on its stream
            _, _, rs = _weight_grads(cell, dgates[l], hseq[l], h0s[l], ins[l], 0, 0, T, dwih=dwih[l], dwhh=dwhh[l],
                                     accumulate=direct[l], pad=True)
            if direct[l]:  # (no copy into dbih first)
                _add_bias_sinks(rs, sinks[l][2], sinks[l][3])
                return
            dbih[l].copy_(rs)
            if cell.db_hh is not None:
                cell.db_hh(rs, dgates[l].view(T * B, 4 * H), H, dbhh[l])

        pipeline_backward(rec, chunks, project, recur, finish)
        dx = None
        if ctx.needs_input_grad[0]:  # (layer 0's stream is the caller's)
            dx = gemm_f32(_cols(dgates[0].view(T * B, 4 * H), 0, xc), False, wp[0], True)[0].view(T, B, I)
        pipeline_join(rec)
        grads: List[Optional[Tensor]] = []
        for l in range(L):
            if direct[l]:  # already accumulated into the parameters' .grad
                grads += [None] * per
                continue
            grads += [dwih[l], dwhh[l]]
            if per == 4:
                grads += [dbih[l] if has_w[l][2] else None, dbhh[l] if has_w[l][3] else None]
        return (dx, *_state_grads(ctx, dhb, dcb if has_c else None, h0_dtype, c0_dtype), None, *grads)


# the name this Function had while it served the LSTM alone: code that wraps
# ``_PipelinedLSTMStack.apply`` to see the pipelined path run keeps working
_PipelinedLSTMStack = _PipelinedStack


def padded_cols(x2: Tensor, mult: int = 32) -> Tensor:
    """x2 [K, n] zero-padded to a multiple of ``mult`` columns (one copy).  A
    weight-gradient GEMM against a narrow, unaligned input (the motion model's
    9 features: rows of 36 bytes) runs gemm_f32's bounds-checked loop, whose
    loads do not overlap its MFMAs; padded, every tile is whole and aligned
    (layer 0's dW_ih 214 -> ~90 us at the motion batch, profiles/r4/gemm_probe/)."""
    n = x2.shape[1]
    shape = (x2.shape[0], -(-n // mult) * mult)
    # the padded buffer is kept per (shape, dtype, device, stream): its pad
    # columns are zeroed once, a step only copies the data columns (one
    # dispatch, not a fill and a copy); reuse is stream-ordered
    if x2.is_cuda and torch.cuda.is_current_stream_capturing():  # (graph-pool memory: never cached)
        out = x2.new_zeros(shape)
        out[:, :n].copy_(x2)
        return out
    key = (shape, x2.dtype, x2.device, torch.cuda.current_stream(x2.device).cuda_stream if x2.is_cuda else 0)
    out = _PADDED.get(key)
    if out is None:
        if len(_PADDED) >= 8:
            _PADDED.clear()
        out = _PADDED[key] = x2.new_zeros(shape)
    out[:, :n].copy_(x2)
    return out


_PADDED: dict = {}


def _chunk_weight_grads(dwih: Tensor, dwhh: Tensor, db: Optional[Tensor], G3: Tensor, hd: Tensor, h0: Optional[Tensor],
                        xin: Tensor, t0: int, t1: int, first: bool) -> Tensor:
    """Steps [t0, t1) of one unidirectional fp32 LSTM layer's dW_ih, dW_hh and
    db, written (first chunk) or accumulated into the fp32 outputs
    (_weight_grads, chunk by chunk; ``db`` None: the row sums as they are)."""
    rs = _weight_grads(LSTM, G3, hd, h0, xin, 0, t0, t1, dwih=dwih, dwhh=dwhh, accumulate=not first, pad=True)[2]
    if db is None:
        return rs
    return db.copy_(rs) if first else db.add_(rs)


# gates i, f, g, o; dgates is gate-blocked, i.e. in parameter order throughout
LSTM = Cell(cell=0, gates=4, has_c=True, xcols=4, hh_blocks=((0, 4, 0),), db_hh=None, shadows=_lstm_shadows,
            backward16=_backward_gemms16)


def large_forward(cell: Cell, x: Tensor, weights: Sequence[Optional[Tensor]], h0: Optional[Tensor],
                  c0: Optional[Tensor], *, hidden: int, num_layers: int, batch_first: bool, bidirectional: bool = False,
                  dropout: float = 0.0, training: bool = False) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """A stacked (bidirectional) RNN of ``cell`` on the MFMA step kernels ->
    (out, hn, cn) as nn.LSTM / nn.GRU return them (cn None without a c state).

    ``weights``: ``_all_weights`` order (per layer and direction w_ih,
    w_hh[, b_ih, b_hh])."""
    ndir = 2 if bidirectional else 1
    per = len(weights) // (num_layers * ndir)
    seq = (x.transpose(0, 1) if batch_first else x).contiguous()  # (a no-op for an index-gathered batch: see lstm_forward)
    if pipeline_ok(seq, hidden, num_layers, bidirectional, dropout, training):
        out, hn, cn = _PipelinedStack.apply(seq, h0, c0, (cell, hidden, num_layers, per, pipeline_chunks(seq.shape[0])),
                                            *weights)
        return (out.transpose(0, 1) if batch_first else out), hn, cn
    tile = _tile()
    hns, cns = [], []
    for l in range(num_layers):
        ws: List[Optional[Tensor]] = []
        for d in range(ndir):
            chunk = list(weights[(l * ndir + d) * per:(l * ndir + d + 1) * per])
            if per == 2:
                chunk += [None, None]
            ws += chunk
        h0l = h0[l * ndir:(l + 1) * ndir] if h0 is not None else None
        c0l = c0[l * ndir:(l + 1) * ndir] if c0 is not None else None
        seq, hn, cn = _LargeLayer.apply(seq, h0l, c0l, (cell, hidden, ndir, tile), *ws)
        hns.append(hn)
        cns.append(cn)
        if dropout > 0 and training and l < num_layers - 1:
            seq = torch.nn.functional.dropout(seq, dropout, True)
    out = seq.transpose(0, 1) if batch_first else seq
    if num_layers == 1:
        return out, hns[0], cns[0]
    if not cell.has_c:  # (slice copies, as the GRU always stacked its states; _StackStates is one pack launch)
        return out, stack_layers(hns), None
    hn, cn = _StackStates.apply(num_layers, *hns, *cns)
    return out, hn, cn


def lstm_large_forward(x: Tensor, weights: Sequence[Optional[Tensor]], h0: Optional[Tensor],
                       c0: Optional[Tensor], **kw) -> Tuple[Tensor, Tensor, Tensor]:
    """Stacked (bi)LSTM on the MFMA step kernels; nn.LSTM-compatible outputs
    (large_forward's keywords)."""
    return large_forward(LSTM, x, weights, h0, c0, **kw)
