"""The wide beam search (csrc/kernels/lstm_decode.hip: Pick::beam in lstm_decode_layer_wide,
lstm_decode_beam_pick_wide; 17 to 64 streams) through ops/decode.py:beam_decode_wide and CharLM.beam_search.

Bit identity with beam_decode on the same prompts in chunks of 16 // W, in everything a search returns and records.
GW: two to four tiles, a partly filled last tile, 64 full streams, groups across one tile boundary (6, 3) and across
every one (9, 7).  In those two the recorded parents must show, after the start, a stream continuing a parent of
another tile: there one epilogue wave's in-place c store would reach another wave's load, were every load not
complete before any store.  (Selection 0 sends every slot to its group's first stream, so position 1 crosses by
construction; the assertion asks for a later one.  The state seed was chosen with the host mirror, beam_reference on the
CPU in fp32: 4 to 44 crossings in each of the 16 (cell, V, layers) x (6, 3), (9, 7) runs.)

Against fp64 in the margin form of tests/_beam_ref.py at V = 256, its eps as it is, the exact fp64 set required on
>= 90 % of the (position, group) triples.  The fp32 host mirror on the same inputs: 78 of 78 triples exact
(smallest boundary gap 1.6e-4, largest eps 4.6e-6); the kernels on an MI355X: 78 of 78 in both dtypes.
"""
import functools

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

import _beam_ref as R
from test_gpu_decode_beam import _assert_guards, _guarded_bufs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
H, E, N = 64, 32, 6
GW = [(17, 1), (6, 3), (2, 9), (9, 7), (3, 16), (4, 16)]
RECORD = ("cum", "done", "tokens", "lp", "parents")
cells = pytest.mark.parametrize("cell", dec.CELLS)
dtypes = pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def _model(cell, cdt, V, L):
    """_beam_ref.lm_model, or the same for a GRU (the head scaled by 8: resolved boundaries)."""
    if cell == "lstm":
        return R.lm_model(H, E, V, L, cdt, seed=V + L, device=DEV)
    torch.manual_seed(V + L)
    model = CharLM(V, E, H, L, compute_dtype=cdt, cell=cell)
    with torch.no_grad():
        model.fc.weight.mul_(8.0)
    return model.to(DEV)


def _inputs(model, G, seed=3):
    """(h0, c0, first): random nonzero entering state of G prompts (a GRU's c0 is None)."""
    g = torch.Generator().manual_seed(seed)
    h0, c0 = (s * torch.randn(model.num_layers, G, H, generator=g) for s in (0.5, 1.0))
    first = torch.randint(0, model.vocab_size, (G,), generator=g).to(DEV)
    return (h0.to(DEV), None, first) if model.cell == "gru" else (h0.to(DEV, model.compute_dtype), c0.to(DEV), first)


def _search(op, model, h0, c0, first, W, bufs=None, **kw):
    """op on these prompts -> (its five results, its buffers with the record)."""
    if bufs is None:
        bufs = dec.alloc_beam_buffers(model.num_layers, first.shape[0], W, H, model.vocab_size, N, model.compute_dtype,
                                      DEV, return_logits=True, return_logprobs=True)
    out = op(model.embedding.weight, model.rnn._weights(), model.fc.weight, model.fc.bias, model.compute_dtype, h0, c0,
             first, N, W, return_logits=True, return_logprobs=True, bufs=bufs, cell=model.cell, **kw)
    return out, bufs


def _assert_chunks_equal(model, h0, c0, first, W, wide, bufs, **kw):
    for g0 in range(0, first.shape[0], dec.MAX_STREAMS // W):
        gs = slice(g0, min(g0 + dec.MAX_STREAMS // W, first.shape[0]))
        ss = slice(gs.start * W, gs.stop * W)  # the chunk's groups and streams
        part, pb = _search(dec.beam_decode, model, h0[:, gs], c0[:, gs] if c0 is not None else None, first[gs], W, **kw)
        for i, (x, y) in enumerate(zip(wide, part)):  # hyp, scores, hyp_lp by group; h, c by stream
            assert torch.equal(x[:, ss] if i >= 3 else x[gs], y), (g0, i)
        for k in RECORD:
            got = bufs[k][:, ss] if k in ("cum", "done") else bufs[k][ss] - (ss.start if k == "parents" else 0)
            assert torch.equal(got, pb[k]), (g0, k)


@pytest.mark.parametrize("G,W", GW)
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("V", [8, 256])
@dtypes
@cells
def test_bits_of_the_16_stream_search(cell, cdt, V, L, G, W):
    model = _model(cell, cdt, V, L)
    h0, c0, first = _inputs(model, G)
    wide, bufs = _search(dec.beam_decode_wide, model, h0, c0, first, W)
    _assert_chunks_equal(model, h0, c0, first, W, wide, bufs)
    if (G, W) in ((6, 3), (9, 7)):  # after the start, a stream continued a parent of another tile
        s = torch.arange(G * W, device=DEV)[:, None]
        assert bool((bufs["parents"][:, 1:] // dec.MAX_STREAMS != s // dec.MAX_STREAMS).any())


@pytest.mark.parametrize("G,W", [(4, 16), (9, 7)])
@dtypes
def test_selections_against_fp64(cdt, G, W):
    model = _model("lstm", cdt, 256, 2)
    _, bufs = _search(dec.beam_decode_wide, model, *_inputs(model, G), W)
    res = R.check_run({k: bufs[k].cpu() for k in RECORD + ("logits",)}, W, None, what=f"{G} x {W}")
    assert len(res) == N * G and sum(r["exact"] for r in res) >= 0.9 * len(res)


@cells
def test_stop_in_guarded_buffers_twice(cell):
    """NaN-filled buffers between guard zones, ``stop`` set: the same bits twice; done and the lengths the chunks'."""
    G, W, V, L, stop = 9, 7, 8, 2, 3
    model = _model(cell, torch.float16, V, L)
    h0, c0, first = _inputs(model, G)
    flats, bufs = _guarded_bufs(L, G, W, H, V, N, torch.float16)
    runs = []
    for _ in range(2):
        out, _ = _search(dec.beam_decode_wide, model, h0, c0, first, W, bufs=bufs, stop=stop)
        torch.cuda.synchronize()
        _assert_guards(flats)
        runs.append([x.clone() for x in out] + [bufs[k].clone() for k in RECORD + ("logits", "hyp", "hyp_lp")])
    for x, y in zip(*runs):
        assert not bool(torch.isnan(x.float()).any()) and torch.equal(x, y)
    _assert_chunks_equal(model, h0, c0, first, W, out, bufs, stop=stop)  # (done is part of the record)
    done, short = bufs["done"][N].bool(), dec.stop_lengths(out[0], stop)[0].view(-1) < N
    assert bool(done.any()) and not bool(done.all()) and bool(short.any()) and torch.equal(short, done & short)


def test_refusals_and_routing(monkeypatch):
    mod = _ext.require()
    ok = (9, 7, 64, 32, 1024, 2, 0)
    for fits in (mod.lstm_decode_beam_wide_supported, mod.gru_decode_beam_wide_supported):
        assert fits(*ok) and fits(64, 1, 1024, 256, 256, 5, 1) and fits(4, 16, 64, 32, 8, 1, 0)
        # G W = 16, G W = 65, W = 0, W = 17, V = 1025, H = 96
        for bad in ((2, 8), (1, 16), (5, 13), (17, 0), (2, 17), (9, 7, 64, 32, 1025), (9, 7, 96)):
            assert not fits(*bad, *ok[len(bad):]), bad
    model = _model("lstm", torch.bfloat16, 8, 2)
    h0, c0, first = _inputs(model, 10)
    big = dec.alloc_beam_buffers(2, 5, 13, H, 8, N, torch.bfloat16, DEV, return_logits=True, return_logprobs=True)
    with monkeypatch.context() as m:  # past the op's own checks: the binding refuses 65 streams
        m.setattr(dec, "check_beam", lambda *a, **k: None)
        m.setattr(dec, "beam_wide_supported", lambda *a, **k: True)
        with pytest.raises(RuntimeError, match="lstm_decode_beam_wide"):
            _search(dec.beam_decode_wide, model, h0[:, :5], c0[:, :5], first[:5], 13, bufs=big)
    for op, g, w in ((dec.beam_decode, 2, 9), (dec.beam_decode_wide, 5, 13)):
        with pytest.raises(ValueError):
            _search(op, model, h0[:, :g], c0[:, :g], first[:g], w)

    calls = []
    for name in ("beam_decode", "beam_decode_wide"):
        real = getattr(dec, name)
        monkeypatch.setattr(dec, name, lambda *a, _r=real, _n=name, **k: (calls.append((_n, a[7].shape[0])), _r(*a, **k))[1])
    kw = dict(state=(h0, c0), return_logprobs=True, return_state=True)
    nine, ten = model.beam_search(first[:9, None], N, 7, **kw), model.beam_search(first[:, None], N, 7, **kw)
    assert calls == [("beam_decode_wide", 9), ("beam_decode_wide", 9), ("beam_decode", 1)]
    for b in range(10):
        one = model.beam_search(first[b:b + 1, None], N, 7, **{**kw, "state": (h0[:, b:b + 1], c0[:, b:b + 1])})
        for out in (nine, ten)[b // 9:]:
            for x, y in zip(one[:4], out[:4]):
                assert torch.equal(x[0], y[b]), b
            for x, y in zip(one[4], out[4]):
                assert torch.equal(x, y[:, b * 7:(b + 1) * 7]), b
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    with pytest.raises(RuntimeError, match="strict"):  # a vocabulary the kernels do not cover
        CharLM(1025, 32, 64, 1, compute_dtype=torch.bfloat16).to(DEV).beam_search(first[:9, None], 2, 7)
