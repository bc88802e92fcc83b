"""CPU checks of the fp32 stacked-layer pipeline's bookkeeping
(ops/lstm_large.py): time chunks and the chunk-by-chunk weight gradients
(the gemm_f32 torch fallback stands in for the HIP GEMM)."""
import pytest
import torch

from pytorch_distributed_rnn_amd.ops.gru_large import GRU
from pytorch_distributed_rnn_amd.ops.lstm_large import LSTM, _chunk_weight_grads, _weight_grads, pipeline_chunks

from _tune import set_tune


def test_pipeline_chunks_cover_the_sequence(monkeypatch):
    for c, T in [(4, 128), (3, 10), (16, 12), (1, 5)]:
        set_tune(monkeypatch, large_chunks=str(c))
        ch = pipeline_chunks(T)
        assert len(ch) == min(c, T) and ch[0][0] == 0 and ch[-1][1] == T
        assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ch, ch[1:]))


@pytest.mark.parametrize("chunks", [1, 2, 3, 7])
@pytest.mark.parametrize("with_h0", [False, True])
def test_chunked_weight_grads_match_whole_sequence(chunks, with_h0, monkeypatch):
    torch.manual_seed(0)
    T, B, H, I = 7, 3, 8, 5
    G = torch.randn(T, B, 4 * H)
    hd = torch.randn(T, B, H)
    x = torch.randn(T, B, I)
    h0 = torch.randn(B, H) if with_h0 else None
    set_tune(monkeypatch, large_chunks=str(chunks))
    dwih, dwhh, db = torch.full((4 * H, I), float("nan")), torch.full((4 * H, H), float("nan")), torch.empty(4 * H)
    for k, (t0, t1) in enumerate(reversed(pipeline_chunks(T))):  # the backward's order: last chunk first
        _chunk_weight_grads(dwih, dwhh, db, G, hd, h0, x, t0, t1, k == 0)
    hprev = torch.cat([(h0 if h0 is not None else torch.zeros(B, H))[None], hd[:-1]], 0)
    G2 = G.reshape(-1, 4 * H)
    torch.testing.assert_close(dwhh, G2.t() @ hprev.reshape(-1, H), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dwih, G2.t() @ x.reshape(-1, I), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(db, G2.sum(0), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("mode", ["fresh", "chunks"])
@pytest.mark.parametrize("I", [5, 32])
@pytest.mark.parametrize("T,with_h0", [(1, False), (1, True), (7, False), (7, True)])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("cell", [LSTM, GRU], ids=["lstm", "gru"])
def test_weight_grads_match_dense_products(cell, d, T, with_h0, I, mode, monkeypatch):
    """The shared fp32 weight-gradient helper against dense G^T h_prev, G^T x
    and G.sum(0): both cells, both directions (reverse: h_prev(t) = h_{t+1},
    h0 pairs with the last step), T = 1 with and without h0 (the degenerate
    branches, zero fill included), a narrow (padded) and an aligned input;
    "fresh": one call returning new tensors (the layer's use), "chunks":
    written, then accumulated, chunk by chunk into given ones (the stack's)."""
    torch.manual_seed(1)
    B, H = 3, 8
    G = torch.randn(T, B, 4 * H)
    hd = torch.randn(T, B, H)
    x = torch.randn(T, B, I)
    h0 = torch.randn(B, H) if with_h0 else None
    R, xc = cell.gates * H, cell.xcols * H
    if mode == "fresh":
        dwih, dwhh, rs = _weight_grads(cell, G, hd, h0, x, d, 0, T)
    else:
        set_tune(monkeypatch, large_chunks="3")
        dwih, dwhh, rs = torch.full((R, I), float("nan")), torch.full((R, H), float("nan")), torch.zeros(xc)
        for k, (t0, t1) in enumerate(reversed(pipeline_chunks(T))):
            a, b, r = _weight_grads(cell, G, hd, h0, x, d, t0, t1, dwih=dwih, dwhh=dwhh, accumulate=k > 0, pad=True)
            assert a is dwih and b is dwhh
            rs += r
    edge = (h0 if with_h0 else torch.zeros(B, H))[None]
    hprev = torch.cat([edge, hd[:-1]], 0) if d == 0 else torch.cat([hd[1:], edge], 0)
    G2 = G.reshape(-1, 4 * H)
    dense_hh, col = G2.t() @ hprev.reshape(-1, H), G2.sum(0)
    if cell is GRU:  # nn.GRU's layout: the quad [r | z | n_x | n_h] without its n_x block
        dense_hh, col_hh = torch.cat([dense_hh[:2 * H], dense_hh[3 * H:]]), torch.cat([col[:2 * H], col[3 * H:]])
    assert dwih.shape == (R, I) and dwhh.shape == (R, H) and rs.shape == (xc,)
    torch.testing.assert_close(dwhh, dense_hh, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dwih, G2[:, :xc].t() @ x.reshape(-1, I), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rs, col[:xc], rtol=1e-5, atol=1e-5)
    if cell is GRU:
        db_hh = cell.db_hh(rs, G2, H, torch.full((R,), float("nan")))
        torch.testing.assert_close(db_hh, col_hh, rtol=1e-5, atol=1e-5)
    else:
        assert cell.db_hh is None  # db_hh is db_ih, the row sums themselves
