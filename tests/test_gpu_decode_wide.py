"""The wide-tile decode kernels (csrc/kernels/lstm_decode.hip: lstm_decode_layer_wide,
lstm_decode_head_wide; 17 to 64 streams per launch) through ops/decode.py and
CharLM.generate.

Per position against the fp64 references of tests/_decode_ref.py and
tests/_gru_decode_ref.py, teacher-forced as in test_gpu_decode.py, under
_decode_ref.bound = 2e-5 + (1e-4 + r) |ref| (r: 2^-8 for bf16 h, 2^-11 for fp16
h; for the fp32 values 0 on the LSTM and 2^-24 on the GRU, as the 16-stream
tests have it), every buffer between sentinel guard zones.  Then bit for bit
against the 16-stream kernels on row groups of 16: a stream's tokens, logits,
h and c do not depend on how the batch is tiled.

Shapes (cell, H, E, V, layers, B, N):
    lstm  64, 32,  24, 1, 17, 2   one live stream in tile 1
    lstm  64, 32,   8, 2, 33, 3   three tiles, odd N, cross-layer read
    lstm 192, 96,  40, 3, 64, 2   every tile full, K-split remainder
    lstm 128, 64, 256, 2, 49, 3   nonzero initial state
    gru   64, 32,  40, 2, 33, 3   the GRU cell

Worst |kernel - ref| / bound measured on an MI355X when this file was written:
see profiles/r20/decode_wide.md.
"""
import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

import _decode_ref as R
import _gru_decode_ref as G
from test_gpu_decode_filter import _assert_guards, _guarded_bufs

pytestmark = pytest.mark.gpu

CASES = [("lstm", 64, 32, 24, 1, 17, 2), ("lstm", 64, 32, 8, 2, 33, 3), ("lstm", 192, 96, 40, 3, 64, 2),
         ("lstm", 128, 64, 256, 2, 49, 3), ("gru", 64, 32, 40, 2, 33, 3)]
ULP_HALF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DEV = torch.device("cuda", 0)
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-H{}E{}V{}L{}B{}N{}".format(*c))
dtypes = pytest.mark.parametrize("cdt", list(ULP_HALF), ids=["bf16", "fp16"])


def _setup(case, cdt):
    """(model, h0, c0, first): the GRU's and the last LSTM case's entering state nonzero (a GRU's c0 is None)."""
    cell, H, E, V, L, B, _ = case
    g = torch.Generator().manual_seed(H + V + B)
    if cell == "gru":
        model = G.gru_model(H, E, L, cdt, DEV, V=V)
    else:
        torch.manual_seed(0)
        model = CharLM(V, E, H, L, compute_dtype=cdt).to(DEV)
    h0 = c0 = None
    if cell == "gru" or case == CASES[3]:
        h0 = (0.5 * torch.randn(L, B, H, generator=g)).to(DEV)
        h0, c0 = (h0, None) if cell == "gru" else (h0.to(cdt), torch.randn(L, B, H, generator=g).to(DEV))
    return model, h0, c0, torch.randint(0, V, (B,), generator=g).to(DEV)


def _low(model, h0, c0, first, N, **kw):
    return dec.decode(model.embedding.weight, model.rnn._weights(), model.fc.weight, model.fc.bias,
                      model.compute_dtype, h0, c0, first, N, cell=model.cell, **kw)


@dtypes
@cases
def test_positions_against_fp64(case, cdt):
    cell, H, E, V, L, B, N = case
    model, h0, c0, first = _setup(case, cdt)
    gru = cell == "gru"
    w = (G if gru else R).weights_of(model, cdt)
    forced = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(B)).to(DEV)
    zeros = torch.zeros(L, B, H, device=DEV)
    h = (h0 if h0 is not None else zeros).to(cdt)                 # the 16-bit h entering the position
    c = h0 if gru else (c0 if c0 is not None else zeros)          # the fp32 state: c, or the GRU's master of h
    worst = {"h": 0.0, "c": 0.0, "logits": 0.0}
    steps = []
    for p in range(N):  # one position per call: every position's h, c and logits against the reference
        flats, bufs = _guarded_bufs(L, B, H, V, 1, cdt)
        tok, lg, hn, cn = _low(model, c if gru else h, None if gru else c, first, 1, bufs=bufs, seed=11, pos0=1 + p,
                               forced=forced[:, p:p + 1], return_logits=True)
        torch.cuda.synchronize()
        _assert_guards(flats)
        if gru:
            rh, rl = G.position(w, c, forced[:, p], h_own=hn, h_read=h)
            rc, r32 = rh, 2.0 ** -24
        else:
            rh, rc, rl = R.position(w, h, c, forced[:, p], h_own=hn)
            r32 = 0.0
        for name, got, ref, r in (("h", hn, rh, ULP_HALF[cdt]), ("c", cn, rc, r32), ("logits", lg[:, 0], rl, r32)):
            assert got.shape == ref.shape
            worst[name] = max(worst[name], R.worst(got, ref, r))
        steps.append((tok.clone(), lg.clone()))
        h, c = hn.clone(), cn.clone()
    print(f"wide decode worst/bound {case} {cdt}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # all N positions in one call: the same bits (the ping-pong's parity), nothing outside the buffers
    flats, bufs = _guarded_bufs(L, B, H, V, N, cdt)
    tok, lg, hn, cn = _low(model, h0, c0, first, N, bufs=bufs, seed=11, pos0=1, forced=forced, return_logits=True)
    torch.cuda.synchronize()
    _assert_guards(flats)
    assert torch.equal(tok, torch.cat([s[0] for s in steps], 1)) and torch.equal(lg, torch.cat([s[1] for s in steps], 1))
    assert torch.equal(hn, h) and torch.equal(cn, c)
    assert int(tok.min()) >= 0 and int(tok.max()) < V


@pytest.mark.parametrize("mode", ["sample", "greedy", "filtered"])
@dtypes
@cases
def test_bits_of_the_16_stream_kernels(case, cdt, mode):
    """One wide call, free running, against 16-stream calls on row groups of 16 with stream0 = the group's first row."""
    _, H, E, V, L, B, N = case
    model, h0, c0, first = _setup(case, cdt)
    kw = dict(temperature=0.0 if mode == "greedy" else 1.0, seed=5, pos0=1, return_logits=True)
    if mode == "filtered":
        kw.update(top_k=5, top_p=0.9, return_threshold=True, return_logprobs=True)
    wide = [x.clone() for x in _low(model, h0, c0, first, N + 1, **kw)]
    for b0 in range(0, B, dec.MAX_STREAMS):
        rows = slice(b0, min(b0 + dec.MAX_STREAMS, B))
        part = _low(model, h0[:, rows] if h0 is not None else None, c0[:, rows] if c0 is not None else None,
                    first[rows], N + 1, stream0=b0, **kw)
        for i, (got, want) in enumerate(zip(wide, part)):
            assert torch.equal(got[:, rows] if i in (2, 3) else got[rows], want), (b0, i)
    assert not torch.equal(wide[1][0], wide[1][B - 1])  # (the streams are not copies of one)


def test_refusals_and_routing(monkeypatch):
    mod = _ext.require()
    ok = (64, 64, 32, 1024, 2, 0)
    for fits in (mod.lstm_decode_wide_supported, mod.gru_decode_wide_supported):
        assert fits(*ok) and fits(17, 1024, 256, 256, 5, 1)
        for k, bad in ((0, 16), (0, 65), (2, 48), (3, 1025), (5, 2)):  # B = 16, B = 65, E = 48, V = 1025, fp32
            assert not fits(*ok[:k], bad, *ok[k + 1:]), (k, bad)
    H, E, V, L, N = 64, 32, 24, 2, 3
    torch.manual_seed(0)
    model = CharLM(V, E, H, L, compute_dtype=torch.bfloat16).to(DEV)
    prompt = torch.randint(0, V, (80, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    calls, real = [], dec.decode
    monkeypatch.setattr(dec, "decode", lambda *a, **k: (calls.append(a[7].shape[0]), real(*a, **k))[1])
    kw = dict(temperature=1.0, seed=9, return_logits=True)
    t80, l80 = model.generate(prompt, N, **kw)
    assert calls == [64, 16]  # one wide call, the remainder on the 16-stream kernels
    t64, l64 = model.generate(prompt[:64], N, **kw)
    t16, l16, _, _ = _low(model, None, None, prompt[64:, 0], N, stream0=64, pos0=1, **kw)
    assert torch.equal(t80, torch.cat([t64, t16])) and torch.equal(l80, torch.cat([l64, l16]))
    # B = 16 never reaches the wide op
    del calls[:]
    monkeypatch.setattr(mod, "lstm_decode_wide", None)
    t, l = model.generate(prompt[:16], N, **kw)
    assert calls == [16] and torch.equal(t, t80[:16]) and torch.equal(l, l80[:16])
