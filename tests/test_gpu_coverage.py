"""GPU: configurations the reference CLI accepts (any --hidden-units /
--stacked-layer into nn.LSTM, reference src/motion/main.py:20-21,
src/motion/model.py:9) run on the HIP kernels -- zero-padded hidden units,
layer chunks, per-direction bidirectional launches, dropout between layer
chunks, fp32 large hidden sizes on the MFMA step kernels -- under strict kernel mode (PDRNN_KERNELS=hip-strict: an ATen/MIOpen
fallback raises), checked against fp64 torch modules."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")


def _check(mod_ref, mod, x, h0=None, tol=2e-4):
    out_ref, st_ref = mod_ref(x, h0) if h0 is not None else mod_ref(x)
    hn_ref = st_ref[0] if isinstance(st_ref, tuple) else st_ref
    g = torch.randn_like(out_ref)
    ((out_ref * g).sum() + hn_ref.square().sum()).backward()
    dev = torch.device("cuda")
    xg = x.float().to(dev)
    out, st = mod(xg)
    hn = st[0] if isinstance(st, tuple) else st
    err = (out.double().cpu() - out_ref).abs().max().item()
    assert err < tol, err
    assert (hn.double().cpu() - hn_ref).abs().max().item() < tol
    ((out * g.float().to(dev)).sum() + hn.square().sum()).backward()
    for (n, p), q in zip(mod.named_parameters(), mod_ref.parameters()):
        scale = q.grad.abs().max().item() + 1e-6
        e = (p.grad.double().cpu() - q.grad).abs().max().item()
        assert e / scale < 5e-4, (n, e, scale)


@pytest.mark.parametrize("cell,H,L,bidir", [
    ("lstm", 8, 2, False), ("lstm", 48, 2, False), ("lstm", 24, 3, False), ("lstm", 32, 5, False),
    ("lstm", 32, 2, True), ("lstm", 16, 1, True), ("gru", 8, 2, False), ("gru", 48, 3, False),
    # fp32 large-H: MFMA 16x16x4 f32 step kernels (lstm_large.hip, F32 storage);
    # H = 100 is zero-padded to 128
    ("lstm", 128, 2, False), ("lstm", 100, 1, False), ("lstm", 128, 1, True), ("gru", 128, 2, False),
    ("gru", 192, 1, True),
])
def test_uncovered_shapes_run_on_hip(cell, H, L, bidir):
    from pytorch_distributed_rnn_amd.models.rnn import GRU, LSTM
    torch.manual_seed(0)
    I, B, T = 9, 6, 33
    cls_ref = torch.nn.LSTM if cell == "lstm" else torch.nn.GRU
    ref = cls_ref(I, H, L, batch_first=True, bidirectional=bidir).double()
    mod = (LSTM if cell == "lstm" else GRU)(I, H, L, batch_first=True, bidirectional=bidir).cuda()
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    _check(ref, mod, torch.randn(B, T, I, dtype=torch.float64))


@pytest.mark.parametrize("cell,H,L,opt", [
    ("lstm", 24, 3, "state"), ("gru", 8, 2, "state"),          # h0 (and c0) into a padded, chunked stack
    ("lstm", 32, 2, "no_bias"), ("gru", 32, 2, "no_bias"),
    ("lstm", 48, 2, "time_first"),                             # time-first input on a padded stack
    ("lstm", 32, 5, "idx"), ("lstm", 32, 5, "nograd"),         # two chunks: in-kernel gather; need_out=False
])
def test_stack_options_run_on_hip(cell, H, L, opt):
    """What the small-H stack runner passes along besides the shape -- initial
    states, absent biases, the time-first layout, the batch gather (first
    chunk only) and the inference launch that streams no output -- against
    fp64 modules at _check's tolerances, input and state gradients included."""
    from pytorch_distributed_rnn_amd.models.rnn import GRU, LSTM
    torch.manual_seed(0)
    I, B, T = 9, 6, 33
    lstm, dev = cell == "lstm", torch.device("cuda")
    kw = dict(bias=opt != "no_bias", batch_first=opt != "time_first")
    ref = (torch.nn.LSTM if lstm else torch.nn.GRU)(I, H, L, **kw).double()
    mod = (LSTM if lstm else GRU)(I, H, L, **kw).cuda()
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    N = B + 3 if opt == "idx" else B
    x = torch.randn((T, N, I) if opt == "time_first" else (N, T, I), dtype=torch.float64, requires_grad=True)
    idx = torch.randperm(N)[:B] if opt == "idx" else None
    st = [torch.randn(L, B, H, dtype=torch.float64, requires_grad=True) for _ in range(2 if lstm else 1)] \
        if opt == "state" else []
    xg = x.detach().float().to(dev).requires_grad_(idx is None)  # (no input gradient through the gather)
    stg = [s.detach().float().to(dev).requires_grad_() for s in st]

    def hx(s):
        return None if not s else (tuple(s) if lstm else s[0])

    def states(res):
        return list(res) if lstm else [res]

    out_ref, res_ref = ref(x if idx is None else x[idx], hx(st))
    if opt == "nograd":
        with torch.no_grad():
            out, res = mod(xg, need_out=False)
        assert out is None
        for a, b in zip(states(res), states(res_ref)):
            assert (a.double().cpu() - b).abs().max().item() < 2e-4
        return
    out, res = mod(xg, hx(stg), **({"idx": idx.to(dev)} if idx is not None else {}))
    assert (out.double().cpu() - out_ref).abs().max().item() < 2e-4
    for a, b in zip(states(res), states(res_ref)):
        assert (a.double().cpu() - b).abs().max().item() < 2e-4
    g = torch.randn_like(out_ref)
    ((out_ref * g).sum() + sum(s.square().sum() for s in states(res_ref))).backward()
    ((out * g.float().to(dev)).sum() + sum(s.square().sum() for s in states(res))).backward()
    pairs = [(n, p.grad, q.grad) for (n, p), q in zip(mod.named_parameters(), ref.parameters())]
    pairs += [("dx", xg.grad, x.grad)] * (idx is None)
    pairs += [(f"dstate{k}", a.grad, b.grad) for k, (a, b) in enumerate(zip(stg, st))]
    for n, got, want in pairs:
        scale = want.abs().max().item() + 1e-6
        e = (got.double().cpu() - want).abs().max().item()
        assert e / scale < 5e-4, (n, e, scale)


def test_motion_cli_shapes_train_on_hip(tmp_path):
    """main.py-equivalent model builds with the reference's flags train a step
    through the kernels (strict mode), dropout between layer chunks included."""
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    for H, L, bidir in ((48, 2, False), (8, 2, False), (32, 2, True), (128, 2, False), (256, 1, True)):
        torch.manual_seed(1)
        m = MotionModel(9, H, L, 6, bidirectional=bidir).cuda()
        m.lstm.dropout = 0.1
        m.train()
        x = torch.randn(64, 128, 9, device="cuda")
        y = torch.randint(0, 6, (64,), device="cuda")
        loss = torch.nn.functional.cross_entropy(m(x), y)
        loss.backward()
        assert torch.isfinite(loss)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
