"""GPU: the chunked sequence-in-wave forward (kernels/lstm_sw.hip, mode 8:
layer 1's input projection formed per 16-step chunk on the matrix cores, its
per-step VALU work the recurrent half alone) against fp64 and against the
per-step map it derives from (mode 6), whose results it reproduces bit for
bit."""
import copy

import pytest
import torch

from _tune import set_tune

pytestmark = pytest.mark.gpu

H, NL, C = 32, 2, 6
FWD_DEFAULT_HEADLINE = 8  # forward map lstm_head_step_plan picks at B = 1440 / 1152 (profiles/r7/fwd_chunked.md)


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.native(torch.device("cuda", 0))


def _fused_grads(model, train, B, round_bf16=False):
    """Gradients of one fused step (no optimizer update) on the first batch,
    the batch gathered through the loader's index vector."""
    from pytorch_distributed_rnn_amd.ops.lstm import LSTM, step_launch_config
    from pytorch_distributed_rnn_amd.train.trainer import Trainer
    t = Trainer(model, train, batch_size=B, learning_rate=2.5e-3, device=torch.device("cuda"))
    f = t._fused_step()
    assert f is not None
    feats, labels, idx = t.train_loader.make_batch(t.train_loader.batch_indices()[0])
    (nb_f, sp_f), nb_b = step_launch_config(LSTM, idx.numel(), f.H, f.NL)
    ws = f.weights
    if f.gru:
        from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
        ws = _pack(f.weights, f.NL, f.H, f.flat.data)
        nb_f, sp_f = 1, 1
    f.flat.attach_grads()
    f.flat.grad.zero_()
    stats = torch.zeros(3, device="cuda")
    f.mod.lstm_head_train_step(feats, idx, labels, ws, f.m.fc.weight, f.m.fc.bias, f.flat.grad, stats, f.H, f.NL,
                               sp_f, 0, nb_f, nb_b, None, None,
                               1 if f.gru else 0, f.colmap, round_bf16=round_bf16)
    return [p.grad.detach().double() for p in f.m.parameters()], feats.index_select(0, idx), \
        labels.index_select(0, idx).reshape(-1), f.flat.grad.detach().clone()


def _fp64_check(m0, train, B, tol=2e-6, round_bf16=False):
    """Gradients before Adam against fp64 autograd on the same weights and
    batch, each within tol of the parameter's largest gradient (the check and
    tolerance of tests/test_gpu_train.py).  round_bf16: the kernels round the
    recurrent stack's fp32 masters to bf16 as they load them, so the reference
    runs on the rounded values."""
    grads, x, y, _ = _fused_grads(copy.deepcopy(m0), train, B, round_bf16)
    ref = copy.deepcopy(m0).cuda()
    if round_bf16:
        with torch.no_grad():
            for k, p in ref.named_parameters():
                if k.startswith("lstm."):
                    p.copy_(p.to(torch.bfloat16).float())
    ref = ref.double()
    torch.nn.functional.cross_entropy(ref(x.double()), y).backward()
    for (k, r), g in zip(ref.named_parameters(), grads):
        scale = r.grad.abs().max().item()
        err = (g - r.grad).abs().max().item()
        print(f"{k}: err {err:.3e} scale {scale:.3e}")
        assert err <= tol * scale + 1e-12, k


def _data(B, T, seed):
    from pytorch_distributed_rnn_amd.data.motion import synthetic_motion
    train, _, _ = synthetic_motion(n_train=B, n_validation=2, n_test=2, seq_length=T, seed=seed)
    return train


def _model(cell):
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    return MotionModel(9, H, NL, C, cell=cell)


def _plan(T, B, cell):
    return _mod().lstm_head_step_plan(H, 9, NL, T, B, cell=1 if cell == "gru" else 0)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("bwd", ["3", "2"])
@pytest.mark.parametrize("T", [16, 32, 48])
def test_chunk_edges_gradients_match_fp64(T, bwd, cell, monkeypatch):
    """One chunk (the layer-1 wave runs in the drain slot only), two (both
    halves of the h^0 ring) and three (the ring wraps); B = 3: with backward
    map 3 a half-empty two-sequence BPTT wave reads this forward's act / hseq."""
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode="8", sw_bwd_mode=bwd)
    p = _plan(T, 3, cell)
    assert p["sw"] and p["sw_fmode"] == 8 and p["sw_bmode"] == int(bwd), p
    torch.manual_seed(41 + T)
    _fp64_check(_model(cell), _data(3, T, 42), 3)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("round_bf16", [False, True])
def test_headline_length_odd_grid_gradients_match_fp64(round_bf16, cell, monkeypatch):
    """T = 128 (eight chunks) on an odd grid of 97 gathered sequences, fp32
    weights and weights rounded to bf16 as they load (the MFMA B operand too)."""
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode="8", sw_bwd_mode=None)
    assert _plan(128, 97, cell)["sw_fmode"] == 8
    torch.manual_seed(43)
    _fp64_check(_model(cell), _data(97, 128, 44), 97, round_bf16=round_bf16)


def _ref_stack(cell, ws, x):
    """fp64 nn.LSTM / nn.GRU layer by layer on the same weights: every layer's
    h sequence and the rows the forward saves ([B, T, 5, H]: LSTM i, f, g, o, c;
    GRU r, z, n_x, n_h, n), the gates formed in fp64 from the module's own h."""
    hs, acts, inp = [], [], x
    for l in range(NL):
        w_ih, w_hh, b_ih, b_hh = [w.double() for w in ws[4 * l:4 * l + 4]]
        rnn = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(inp.shape[-1], H, 1, batch_first=True).cuda().double()
        with torch.no_grad():
            for p, q in zip(rnn.parameters(), (w_ih, w_hh, b_ih, b_hh)):
                p.copy_(q)
            out = rnn(inp)[0]
        hprev = torch.cat([torch.zeros_like(out[:, :1]), out[:, :-1]], 1)
        gi, gh = inp @ w_ih.T + b_ih, hprev @ w_hh.T + b_hh
        if cell == "gru":
            (ir, iz, inn), (hr, hz, hn) = gi.chunk(3, -1), gh.chunk(3, -1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            acts.append(torch.stack([r, z, inn, hn, torch.tanh(inn + r * hn)], 2))
        else:
            i, f, g, o = (gi + gh).chunk(4, -1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c, cs = torch.zeros_like(i[:, 0]), []
            for t in range(inp.shape[1]):
                c = f[:, t] * c + i[:, t] * g[:, t]
                cs.append(c)
            acts.append(torch.stack([i, f, g, o, torch.stack(cs, 1)], 2))
        hs.append(out)
        inp = out
    return torch.stack(hs), torch.stack(acts)


def _direct_errors(I, cell, bf16):
    """Largest |error| over hseq and act of forward maps 6 and 8 against fp64
    on the same inputs.  bf16: a bf16 input and the weights rounded to bf16 as
    they load; the reference runs on the rounded values."""
    mod = _mod()
    torch.manual_seed(45 + I)
    rnn = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(I, H, NL, batch_first=True).cuda()
    ws = [p.detach() for p in rnn.parameters()]
    x = torch.randn(2, 32, I, device="cuda")
    if bf16:
        x = x.to(torch.bfloat16)
    kw = ws
    if cell == "gru":
        from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
        kw = _pack(ws, NL, H, ws[0])
    ws_ref = [w.to(torch.bfloat16).float() for w in ws] if bf16 else ws
    h_ref, a_ref = _ref_stack(cell, ws_ref, x.double())
    err = {}
    for mode in (6, 8):
        hseq, act, _, _ = mod.lstm_sw_fwd(x, kw, H, NL, mode, cell=1 if cell == "gru" else 0, round_bf16=bf16)
        eh, ea = (hseq.double() - h_ref).abs().max().item(), (act.double() - a_ref).abs().max().item()
        print(f"I={I} {cell} bf16={bf16} mode {mode}: hseq err {eh:.3e} act err {ea:.3e}")
        err[mode] = max(eh, ea)
    return err


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("I", [1, 9, 12])
def test_input_widths_within_twice_the_per_step_maps_error(I, cell):
    """Input widths 1, 9 and 12 (the widest the family serves: the MFMA K
    range of the per-step layer 0 full) through the direct forward: hseq and act against fp64, the
    chunked map's largest error at most twice the per-step map's on the same
    inputs (both are fp32 sums of at most 64 exact products per gate; only the
    association differs)."""
    err = _direct_errors(I, cell, False)
    assert err[6] < 1e-5, err  # the yardstick itself is at fp32 round-off
    assert err[8] <= 2 * err[6], err


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_bf16_input_and_weights_keep_their_meaning(cell):
    """Both bf16 switches on the chunked map: a bf16 input (read by the lanes
    as MFMA A values) and weights rounded to bf16 as they load (the MFMA B
    fragments and the biases included), against fp64 on the rounded values;
    the same bound as above."""
    err = _direct_errors(9, cell, True)
    assert err[6] < 1e-5, err
    assert err[8] <= 2 * err[6], err


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("B,T,I,bf16", [(2, 32, 9, False), (3, 48, 12, True), (97, 128, 9, False)])
def test_chunked_map_reproduces_the_per_step_map_bit_for_bit(B, T, I, bf16, cell):
    """Every gate pre-activation of mode 8 is the same sequence of fp32
    operations as mode 6's (the even- and odd-column MFMA chains are its two
    v_pk_fma_f32 accumulator halves), so hseq, act, h_n and c_n are
    bit-identical: a model trained on one map is the model trained on the
    other."""
    mod = _mod()
    torch.manual_seed(53 + T)
    rnn = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(I, H, NL, batch_first=True).cuda()
    ws = [p.detach() for p in rnn.parameters()]
    if cell == "gru":
        from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
        ws = _pack(ws, NL, H, ws[0])
    x = torch.randn(B, T, I, device="cuda")
    if bf16:
        x = x.to(torch.bfloat16)
    out = {m: mod.lstm_sw_fwd(x, ws, H, NL, m, cell=1 if cell == "gru" else 0, round_bf16=bf16) for m in (6, 8)}
    for k, (a, b) in enumerate(zip(out[6], out[8])):
        assert torch.equal(a, b), (k, (a - b).abs().max().item())


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_partial_chunk_falls_back_to_per_step_map(cell, monkeypatch):
    """T = 20 is no whole number of chunks: the plan reports forward map 6 and
    the step still matches fp64.  So does the plan for T = 272, whose staged x
    rows would not let six workgroups share a CU (256 is the longest served)."""
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode="8", sw_bwd_mode=None)
    assert _plan(256, 3, cell)["sw_fmode"] == 8 and _plan(272, 3, cell)["sw_fmode"] == 6
    p = _plan(20, 3, cell)
    assert p["sw"] and p["sw_fmode"] == 6, p
    torch.manual_seed(47)
    _fp64_check(_model(cell), _data(3, 20, 48), 3)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_chunked_forward_is_deterministic(cell, monkeypatch):
    """The same step twice: bit-identical hseq, act and flat gradient."""
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode="8", sw_bwd_mode=None)
    torch.manual_seed(49)
    m0, train = _model(cell), _data(3, 32, 50)
    flats, saved = [], []
    for _ in range(2):
        torch.manual_seed(51)  # (the loader's shuffle: the same batch order both times)
        m = copy.deepcopy(m0)
        _, x, _, flat = _fused_grads(m, train, 3)
        flats.append(flat)
        ws = [p.detach() for p in m.lstm.parameters()]
        if cell == "gru":
            from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
            ws = _pack(ws, NL, H, x)
        saved.append(_mod().lstm_sw_fwd(x.contiguous(), ws, H, NL, 8, cell=1 if cell == "gru" else 0)[:2])
    assert torch.equal(flats[0], flats[1])
    assert torch.equal(saved[0][0], saved[1][0]) and torch.equal(saved[0][1], saved[1][1])


def test_default_forward_map_selection(monkeypatch):
    """The headline batches take the map the measurement chose; the smaller
    per-rank batches keep theirs (one wave per SIMD or less: mode 2; two
    workgroups per CU or less: the four-wave mode 5)."""
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode=None, sw_bwd_mode=None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (1440, 1152):
        want = FWD_DEFAULT_HEADLINE if B > 4 * cus else 2 if 2 * B > 4 * cus else 5
        assert _plan(128, B, "lstm")["sw_fmode"] == want, B
    for B in (720, 180):
        want = 6 if B > 4 * cus else 2 if 2 * B > 4 * cus else 5
        assert _plan(128, B, "lstm")["sw_fmode"] == want, B
