"""The small-H stack runner (ops/lstm.py:run_small_stack) on the CPU, with the
ATen cell standing in for the HIP launch: zero-padding of hidden units (how
the fused kernels serve hidden sizes they are not instantiated for,
small_plan), layer chunks, initial states and their slicing are exact -- the
runner reproduces the unpadded fp64 module's outputs, states and every
gradient, and padded units stay exactly zero.  Plus the fused training step's
launch config table (ops/lstm.py:step_launch_config)."""
import pytest
import torch

from pytorch_distributed_rnn_amd.ops.lstm import GRU, LSTM, run_small_stack, step_launch_config

B, T = 3, 7


@pytest.mark.parametrize("batch_first", [True, False], ids=["batch-first", "time-first"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("H,HP,I,L,chunks", [(24, 32, 5, 3, [(0, 2), (2, 1)]), (8, 16, 9, 2, [(0, 1), (1, 1)]),
                                             (32, 32, 9, 5, [(0, 4), (4, 1)]), (48, 64, 9, 1, [(0, 1)])])
@pytest.mark.parametrize("cell", [LSTM, GRU], ids=["lstm", "gru"])
def test_runner_matches_module(cell, H, HP, I, L, chunks, bias, batch_first):
    torch.manual_seed(0)
    mod = (torch.nn.LSTM if cell.has_c else torch.nn.GRU)(I, H, L, bias=bias, batch_first=batch_first).double()

    def inputs():
        x = torch.randn((B, T, I) if batch_first else (T, B, I), dtype=torch.float64)
        return [x] + [torch.randn(L, B, H, dtype=torch.float64) for _ in range(2 if cell.has_c else 1)]

    def loss(out, hn, cn):
        return out.square().sum() + hn.sum() + (cn.square().sum() if cn is not None else 0.0)

    ins = [t.requires_grad_() for t in inputs()]
    ins_ref = [t.detach().clone().requires_grad_() for t in ins]
    out_ref, st = mod(ins_ref[0], tuple(ins_ref[1:]) if cell.has_c else ins_ref[1])
    hn_ref, cn_ref = st if cell.has_c else (st, None)
    loss(out_ref, hn_ref, cn_ref).backward()
    ref_g = [p.grad.clone() for p in mod.parameters()]
    for p in mod.parameters():
        p.grad = None

    launched = []

    def aten(c, x, idx, h0, c0, ws, hidden, n, bf, need_out):
        assert c is cell and idx is None and hidden == HP and bf == batch_first and need_out
        flat = [w for w in ws if w is not None]
        assert len(flat) == (4 if bias else 2) * n
        if c.has_c:
            out, hn, cn = torch._VF.lstm(x, (h0, c0), flat, bias, n, 0.0, False, False, bf)
        else:
            (out, hn), cn = torch._VF.gru(x, h0, flat, bias, n, 0.0, False, False, bf), None
        launched.append((n, out))
        return out, hn, cn

    ws = [getattr(mod, f"{n}_l{l}", None) for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    out, hn, cn = run_small_stack(cell, ins[0], ws, ins[1], ins[2] if cell.has_c else None, (HP, chunks),
                                  hidden=H, batch_first=batch_first, launch=aten)
    assert [n for n, _ in launched] == [n for _, n in chunks]
    for _, o in launched:
        assert o.shape[-1] == HP and torch.equal(o[..., H:], torch.zeros_like(o[..., H:]))
    torch.testing.assert_close(out, out_ref)
    torch.testing.assert_close(hn, hn_ref)
    assert (cn is None) == (cn_ref is None)
    if cn is not None:
        torch.testing.assert_close(cn, cn_ref)
    loss(out, hn, cn).backward()
    for p, g in zip(mod.parameters(), ref_g):
        torch.testing.assert_close(p.grad, g)
    for got, want in zip(ins, ins_ref):  # dx, dh0, dc0
        torch.testing.assert_close(got.grad, want.grad)


# ((nb_fwd, split_fwd), nb_bwd) as the fused step launched before one function
# chose them: the 2-lane K-split forward above B = 1024 at H = 32 only
@pytest.mark.parametrize("tune,cell,batch,H,want", [
    ("", LSTM, 180, 32, ((1, 0), 1)), ("", LSTM, 1024, 32, ((1, 0), 1)), ("", LSTM, 1025, 32, ((1, 2), 1)),
    ("", LSTM, 1440, 32, ((1, 2), 1)), ("", LSTM, 1440, 16, ((1, 0), 1)),
    ("nb_fwd=2", LSTM, 1440, 32, ((2, 0), 1)), ("split_fwd=1", LSTM, 1440, 32, ((1, 1), 1)),
    ("nb_bwd=3", LSTM, 1440, 32, ((1, 2), 3)), ("nb_fwd=2,split_fwd=1,nb_bwd=3", LSTM, 180, 32, ((2, 1), 3)),
    ("nb_fwd=3,nb_bwd=4", LSTM, 1440, 32, ((1, 2), 1)), ("nb_fwd=x,nb_bwd=", LSTM, 180, 32, ((1, 0), 1)),
    ("split_bwd=2", LSTM, 1440, 32, ((1, 2), 1)),
    ("", GRU, 1440, 32, ((1, 1), 1)), ("", GRU, 180, 16, ((1, 1), 1)), ("nb_fwd=2", GRU, 1440, 32, ((2, 1), 1)),
    ("nb_fwd=3,split_fwd=2,nb_bwd=2", GRU, 1440, 32, ((1, 1), 2)),
])
def test_step_launch_config_table(monkeypatch, tune, cell, batch, H, want):
    monkeypatch.setenv("PDRNN_TUNE", tune)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # GRU: the residency rule needs a device
    assert step_launch_config(cell, batch, H, 2, None) == want
