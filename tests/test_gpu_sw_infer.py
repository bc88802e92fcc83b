"""GPU: the inference builds of the sequence-in-wave forward (kernels/lstm_sw.hip,
pdrnn_lstm_sw_infer): the same bits as the training forward in every map, the
head's logits / predictions / statistics, batches beyond the training
family's limit, the plan, the refusals, and the model- and trainer-level
entry points built on them (MotionModel.predict, MotionEvalStep,
Trainer._evaluate)."""
import logging
import math

import pytest
import torch

from _tune import set_tune

pytestmark = pytest.mark.gpu

H = 32
MAPS = {1: (0, 1), 2: (2, 5, 6, 8)}  # forward maps the table lists per layer count
U = 2.0 ** -24                       # fp32 unit roundoff


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.native(torch.device("cuda", 0))


def _stack(cell, I, NL, seed, hidden=H):
    """Weights of a seeded nn.LSTM / nn.GRU as the kernels read them (the GRU
    packed into its 4-block stack)."""
    torch.manual_seed(seed)
    rnn = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(I, hidden, NL, batch_first=True).cuda()
    ws = [p.detach() for p in rnn.parameters()]
    if cell == "gru":
        from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
        ws = _pack(ws, NL, hidden, ws[0])
    return ws


def _head(C, seed, bias=True):
    torch.manual_seed(seed)
    fc = torch.nn.Linear(H, C).cuda()
    return fc.weight.detach().contiguous(), (fc.bias.detach().contiguous() if bias else None)


def _infer(x, ws, hw, hb, NL, cell, labels=None, idx=None, mode=-1, round_bf16=False, need_state=True):
    return _mod().lstm_head_infer(x, idx, labels, ws, hw, hb, H, NL, cell=1 if cell == "gru" else 0,
                                  round_bf16=round_bf16, mode=mode, need_state=need_state)


def _same_state(x, ws, NL, cell, mode, round_bf16=False, idx=None):
    hw, hb = _head(6, 5)
    _, _, _, hn, cn = _infer(x, ws, hw, hb, NL, cell, idx=idx, mode=mode, round_bf16=round_bf16)
    xt = x if idx is None else x.index_select(0, idx).contiguous()
    ref = _mod().lstm_sw_fwd(xt, ws, H, NL, mode, cell=1 if cell == "gru" else 0, round_bf16=round_bf16)[2:]
    assert torch.equal(hn, ref[0]) and torch.equal(cn, ref[1]), \
        (mode, tuple(x.shape), (hn - ref[0]).abs().max().item(), (cn - ref[1]).abs().max().item())


# ------------------------------------------------------------ same bits as training
@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("NL,mode", [(nl, m) for nl, ms in MAPS.items() for m in ms])
def test_state_is_the_training_forwards_bits(NL, mode, cell):
    """h_n / c_n of every inference map equal the training forward's in the
    same map.  B = 3: a half-empty two-sequence wave on map 1; map 8: one
    chunk, both ring halves, ring wrap."""
    for I in (1, 9, 12):
        ws = _stack(cell, I, NL, 10 + I)
        for T in ((16, 32, 48) if mode == 8 else (1, 2, 33)):
            for B in (1, 3):
                torch.manual_seed(100 * T + B)
                _same_state(torch.randn(B, T, I, device="cuda"), ws, NL, cell, mode)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("NL,mode", [(nl, m) for nl, ms in MAPS.items() for m in ms])
def test_state_bits_bf16_and_gathered_headline_length(NL, mode, cell):
    """bf16 x with the weights rounded to bf16 as they load; T = 128 on an odd
    grid of 97 sequences gathered through a permuted index from a 128-row table."""
    ws = _stack(cell, 9, NL, 21)
    torch.manual_seed(22)
    _same_state(torch.randn(3, 32, 9, device="cuda").to(torch.bfloat16), ws, NL, cell, mode, round_bf16=True)
    table = torch.randn(128, 128, 9, device="cuda")
    idx = torch.randperm(128, device="cuda")[:97].contiguous()
    _same_state(table, ws, NL, cell, mode, idx=idx)


# ------------------------------------------------------------ logits
def _logits_bound(hw, hb, h):
    """Any-order bound for 32 rounded products, their sum and the bias add."""
    mag = (hw.double().abs().unsqueeze(0) * h.double().abs().unsqueeze(1)).sum(2)
    if hb is not None:
        mag = mag + hb.double().abs()
    return 34 * U * mag


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("C", [1, 6, 16])
def test_logits_against_fp64_on_the_kernels_own_state(C, bias):
    hw, hb = _head(C, 30 + C, bias)
    for cell in ("lstm", "gru"):
        for NL, modes in MAPS.items():
            ws = _stack(cell, 9, NL, 31)
            for mode in modes:
                torch.manual_seed(32 + mode)
                x = torch.randn(5, 16, 9, device="cuda")
                logits, _, stats, hn, _ = _infer(x, ws, hw, hb, NL, cell, mode=mode)
                assert stats is None and logits.shape == (5, C)
                ref = hn[-1].double() @ hw.double().t()
                if hb is not None:
                    ref = ref + hb.double()
                err = (logits.double() - ref).abs()
                bound = _logits_bound(hw, hb, hn[-1])
                print(f"C={C} bias={bias} {cell} map {mode}: max err {err.max().item():.3e} "
                      f"(bound {bound.min().item():.3e} .. {bound.max().item():.3e})")
                assert bool((err <= bound).all()), (cell, mode)


# ------------------------------------------------------------ predictions and statistics
def _lowest_argmax(logits):
    C = logits.shape[1]
    cols = torch.arange(C, device=logits.device).expand_as(logits)
    return torch.where(logits == logits.max(1, keepdim=True).values, cols, C).min(1).values


def _ulp(v):
    return 2.0 ** (math.floor(math.log2(abs(v))) - 23)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("NL,mode", [(nl, m) for nl, ms in MAPS.items() for m in ms])
def test_predictions_and_sequence_statistics(NL, mode, cell):
    """B = 8 (1 / B exact, so seq_stats[:, 0] * B is the kernel's loss
    itself), labels gathered through the index like the train step's."""
    B, C, N = 8, 6, 12
    ws = _stack(cell, 9, NL, 41)
    hw, hb = _head(C, 42)
    torch.manual_seed(43 + mode)
    table = torch.randn(N, 16, 9, device="cuda")
    labels_all = torch.randint(0, C, (N,), device="cuda")
    idx = torch.randperm(N, device="cuda")[:B].contiguous()
    labels = labels_all.index_select(0, idx)
    logits, pred, stats, _, _ = _infer(table, ws, hw, hb, NL, cell, labels=labels_all, idx=idx, mode=mode)
    assert pred.dtype == torch.int64 and torch.equal(pred, _lowest_argmax(logits))
    assert torch.equal(stats[:, 2], (pred == labels).float())
    assert torch.equal(stats[:, 1], torch.ones(B, device="cuda"))
    ref = torch.nn.functional.cross_entropy(logits.double(), labels, reduction="none")
    stock = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    err = ((stats[:, 0] * B).double() - ref).abs().max().item()
    err_stock = (stock.double() - ref).abs().max().item()
    allowed = max(2 * err_stock, 4 * _ulp(logits.abs().max().item()))
    print(f"{cell} map {mode}: loss err {err:.3e}, stock fp32 cross_entropy err {err_stock:.3e}, allowed {allowed:.3e}")
    assert err <= allowed
    # without labels: no statistics, the same logits and predictions
    l2, p2, s2, _, _ = _infer(table, ws, hw, hb, NL, cell, idx=idx, mode=mode)
    assert s2 is None and torch.equal(l2, logits) and torch.equal(p2, pred)


@pytest.mark.parametrize("NL,mode", [(nl, m) for nl, ms in MAPS.items() for m in ms])
def test_ties_take_the_lowest_class(NL, mode):
    ws = _stack("lstm", 9, NL, 51)
    hw, hb = torch.zeros(16, H, device="cuda"), torch.full((16,), 0.25, device="cuda")
    torch.manual_seed(52)
    x = torch.randn(3, 16, 9, device="cuda")
    logits, pred, stats, _, _ = _infer(x, ws, hw, hb, NL, "lstm", labels=torch.zeros(3, dtype=torch.int64, device="cuda"),
                                       mode=mode)
    assert torch.equal(logits, torch.full((3, 16), 0.25, device="cuda"))
    assert torch.equal(pred, torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert torch.equal(stats[:, 2], torch.ones(3, device="cuda"))


# ------------------------------------------------------------ beyond the training family's batch limit
def test_batch_beyond_the_training_limit():
    NL, T, B, N = 2, 128, 13200, 64
    mod = _mod()
    assert not mod.lstm_sw_fits(NL, B, T)
    with pytest.raises(RuntimeError):
        mod.lstm_sw_plan(NL, B, T)
    plan = mod.lstm_sw_infer_plan(NL, B, T)
    assert plan["map"] in MAPS[NL] and plan["nb"] >= 1
    ws = _stack("lstm", 9, NL, 61)
    hw, hb = _head(6, 62)
    torch.manual_seed(63)
    table = torch.randn(N, T, 9, device="cuda")
    idx = (torch.arange(B, device="cuda") % N).contiguous()
    big = _infer(table, ws, hw, hb, NL, "lstm", idx=idx, need_state=False)
    assert big[3] is None and big[4] is None
    small = _infer(table, ws, hw, hb, NL, "lstm", mode=plan["map"], need_state=False)
    assert torch.equal(big[0], small[0].index_select(0, idx))
    assert torch.equal(big[1], small[1].index_select(0, idx))


# ------------------------------------------------------------ plan
def test_plan_follows_the_training_forward_thresholds(monkeypatch):
    monkeypatch.delenv("PDRNN_SW", raising=False)
    set_tune(monkeypatch, sw_mode=None, sw_bwd_mode=None)
    mod = _mod()
    for B in (97, 180, 512, 720, 1440):
        assert mod.lstm_sw_infer_plan(2, B, 128, 256)["map"] == mod.lstm_sw_plan(2, B, 128, 256)["fwd_map"], B
        assert mod.lstm_sw_infer_plan(1, B, 128, 256)["map"] == mod.lstm_sw_plan(1, B, 128, 256)["fwd_map"], B
    assert mod.lstm_sw_plan(2, 1440, 128, 256)["fwd_map"] == 8
    assert mod.lstm_sw_infer_plan(2, 1440, 126, 256) == {"map": 6, "nb": 1}
    assert mod.lstm_sw_infer_plan(1, 1440, 128, 256) == {"map": 1, "nb": 2}
    # two sequences' x rows past 64 KiB of LDS: one sequence per wave instead
    assert mod.lstm_sw_infer_plan(1, 1440, 640, 256) == {"map": 1, "nb": 2}
    assert mod.lstm_sw_infer_plan(1, 1440, 700, 256) == {"map": 0, "nb": 1}
    set_tune(monkeypatch, sw_mode="2")
    assert mod.lstm_sw_infer_plan(2, 1440, 128, 256)["map"] == 2
    set_tune(monkeypatch, sw_mode="1")  # a one-layer map: ignored for two layers, honoured for one
    assert mod.lstm_sw_infer_plan(2, 1440, 128, 256)["map"] == 8
    assert mod.lstm_sw_infer_plan(1, 97, 128, 256)["map"] == 1
    set_tune(monkeypatch, sw_mode="3")  # a backward-only map
    assert mod.lstm_sw_infer_plan(2, 180, 128, 256)["map"] == mod.lstm_sw_plan(2, 180, 128, 256)["fwd_map"]


# ------------------------------------------------------------ refusals
def test_unsupported_shapes_raise():
    mod = _mod()
    hw, hb = _head(6, 71)
    x = torch.randn(2, 16, 9, device="cuda")
    ok = _stack("lstm", 9, 2, 72)
    _infer(x, ok, hw, hb, 2, "lstm")  # (the supported neighbour of every case below runs)
    with pytest.raises(RuntimeError, match="H = 32"):
        hw16 = torch.zeros(6, 16, device="cuda")
        mod.lstm_head_infer(x, None, None, _stack("lstm", 9, 2, 73, hidden=16), hw16, None, 16, 2)
    with pytest.raises(RuntimeError, match="I <= 12"):
        _infer(torch.randn(2, 16, 13, device="cuda"), _stack("lstm", 13, 2, 74), hw, hb, 2, "lstm")
    with pytest.raises(RuntimeError, match="1 or 2 layers"):
        _infer(x, _stack("lstm", 9, 3, 75), hw, hb, 3, "lstm")
    with pytest.raises(RuntimeError, match="classes"):
        hw17, hb17 = _head(17, 76)
        _infer(x, ok, hw17, hb17, 2, "lstm")
    with pytest.raises(RuntimeError, match="LDS"):
        _infer(torch.randn(1, 2048, 9, device="cuda"), ok, hw, hb, 2, "lstm")
    with pytest.raises(RuntimeError):
        mod.lstm_sw_infer_plan(2, 4, 2048)
    with pytest.raises(RuntimeError, match="wave map"):
        _infer(x, ok, hw, hb, 2, "lstm", mode=1)  # a one-layer map forced on two layers


# ------------------------------------------------------------ model and trainer level
def _motion(cell, NL, seed, **kw):
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    torch.manual_seed(seed)
    return MotionModel(9, H, NL, 6, cell=cell, **kw).cuda().eval()


@pytest.mark.parametrize("cell,NL,dropout", [("lstm", 1, 0.0), ("lstm", 2, 0.0), ("gru", 1, 0.0), ("gru", 2, 0.0),
                                             ("lstm", 2, 0.1), ("gru", 2, 0.1)])
def test_model_predict_matches_forward(cell, NL, dropout):
    """|predict - forward| per element within the logits bound, formed from the
    kernel's own top-layer h_T, plus the forward path's own error against fp64
    in that element."""
    import copy
    from pytorch_distributed_rnn_amd.train import fused_eval
    model = _motion(cell, NL, 81, dropout=dropout)
    assert fused_eval.supported(model, torch.device("cuda", 0))
    torch.manual_seed(82)
    x = torch.randn(7, 33, 9, device="cuda")
    ref_model = copy.deepcopy(model).double()
    with torch.no_grad():
        old = model(x)
        ref = ref_model(x.double())
        h_ref = ref_model.lstm(x.double())[1]
        h_ref = (h_ref[0] if isinstance(h_ref, tuple) else h_ref)[-1]
    new = model.predict(x)
    assert new.shape == old.shape and not new.requires_grad
    # the kernel's own h_T: the same launch with the state returned
    ws = [p.detach() for p in model.lstm.parameters()]
    if cell == "gru":
        from pytorch_distributed_rnn_amd.ops.gru_fused import _pack
        ws = _pack(ws, NL, H, ws[0])
    hw, hb = model.fc.weight.detach(), model.fc.bias.detach()
    logits, _, _, hn, _ = _infer(x, ws, hw, hb, NL, cell)
    assert torch.equal(logits, new)
    bound = _logits_bound(hw, hb, hn[-1])
    err_old = (old.double() - ref).abs()
    diff = (new.double() - old.double()).abs()
    # (for information: what the fused recurrence's own error against fp64 does to the logits)
    dh = ((hn[-1].double() - h_ref) @ hw.double().t()).abs()
    print(f"{cell} NL={NL} dropout={dropout}: |predict - forward| max {diff.max().item():.3e}, forward's fp64 error "
          f"max {err_old.max().item():.3e}, logits bound {bound.min().item():.3e} .. {bound.max().item():.3e}, "
          f"|W (h_fused - h_fp64)| max {dh.max().item():.3e}, smallest slack {(bound + err_old - diff).min().item():.3e}")
    assert bool((diff <= bound + err_old).all())
    idx = torch.tensor([4, 0, 6], device="cuda")
    assert torch.equal(model.predict(x, idx=idx), new.index_select(0, idx))


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_sequences_too_long_for_lds_take_model_forward(cell):
    """T = 1400: no wave map holds the x rows, the plan refuses, and predict /
    MotionEvalStep give model.forward's own results instead of raising; T = 700
    on one layer above one wave per SIMD runs map 0 (same bits as forced)."""
    from pytorch_distributed_rnn_amd.train import fused_eval
    model = _motion(cell, 2, 85)
    torch.manual_seed(86)
    x = torch.randn(3, 1400, 9, device="cuda")
    labels = torch.tensor([1, 5, 0], device="cuda")
    with pytest.raises(RuntimeError):
        _mod().lstm_sw_infer_plan(2, 3, 1400)
    with torch.no_grad():
        old = model(x)
    assert torch.equal(model.predict(x), old)
    step = fused_eval.MotionEvalStep(model)
    logits, pred = step(x, labels)
    assert torch.equal(logits, old) and torch.equal(pred, old.argmax(1))
    loss_sum, n, correct, batches = step.result()
    ref = torch.nn.functional.cross_entropy(old.double(), labels).item()
    assert (n, correct, batches) == (3, int((old.argmax(1) == labels).sum()), 1)
    assert abs(loss_sum - ref) <= 16 * U * max(1.0, ref)  # one fp32 cross-entropy of three rows
    if cell == "lstm":
        ws, (hw, hb) = _stack("lstm", 9, 1, 87), _head(6, 88)
        x1 = torch.randn(3, 700, 9, device="cuda")
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        idx = (torch.arange(4 * cus + 2, device="cuda") % 3).contiguous()  # above one wave per SIMD: map 1's range
        assert _mod().lstm_sw_infer_plan(1, idx.numel(), 700)["map"] == 0
        big = _infer(x1, ws, hw, hb, 1, "lstm", idx=idx, need_state=False)[0]
        assert torch.equal(big, _infer(x1, ws, hw, hb, 1, "lstm", mode=0, need_state=False)[0].index_select(0, idx))


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_trainer_evaluate_fused_and_unfused_agree(cell, monkeypatch, caplog):
    """Three validation batches, the last one short: the same correct total,
    the same loss to the 4 decimals the formatter prints, the same lines, and
    one device-to-host read for the whole fused evaluation."""
    from pytorch_distributed_rnn_amd.data.motion import synthetic_motion
    from pytorch_distributed_rnn_amd.train import fused_eval
    from pytorch_distributed_rnn_amd.train.formatter import TrainingMessageFormatter
    from pytorch_distributed_rnn_amd.train.trainer import Trainer
    train, val, _ = synthetic_motion(n_train=48, n_validation=100, n_test=2, seq_length=32, seed=91)
    model = _motion(cell, 2, 92)
    trainer = Trainer(model, train, batch_size=48, learning_rate=2.5e-3, validation_set=val,
                      device=torch.device("cuda"), warmup=False)
    loader = trainer._get_data_loader(val, batch_size=40)
    assert len(loader) == 3
    # no sequence's top two logits lie within the logits bound of each other
    logits = model.predict(val.features.cuda())
    top = logits.double().topk(2, dim=1).values
    bound = (34 * U * (model.fc.weight.double().abs().sum(1) + model.fc.bias.double().abs())).max().item()
    assert (top[:, 0] - top[:, 1]).min().item() > 2 * bound

    reads = {"result": 0, "cpu": 0}
    real_result, real_cpu = fused_eval.MotionEvalStep.result, torch.Tensor.cpu

    def counted_result(self):
        reads["result"] += 1
        return real_result(self)

    def counted_cpu(self, *a, **k):
        reads["cpu"] += 1
        return real_cpu(self, *a, **k)

    monkeypatch.setattr(fused_eval.MotionEvalStep, "result", counted_result)
    fmt = TrainingMessageFormatter(1)
    out = {}
    for name, env in (("fused", "1"), ("forward", "0")):
        monkeypatch.setenv("PDRNN_FUSED_EVAL", env)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            with monkeypatch.context() as mp:
                if name == "fused":
                    mp.setattr(torch.Tensor, "cpu", counted_cpu)
                loss, acc = trainer._evaluate(loader, fmt, epoch=0)
        lines = [r.getMessage() for r in caplog.records if "Evaluation Epoch" in r.getMessage()]
        assert len(lines) == 1
        out[name] = (loss, acc, lines[0])
        print(name, repr(lines[0]))
    assert reads == {"result": 1, "cpu": 1}
    assert out["fused"][1] == out["forward"][1]                         # correct / n
    assert f"{out['fused'][0]:.4f}" == f"{out['forward'][0]:.4f}"
    assert out["fused"][2] == out["forward"][2]
    n_correct = round(out["fused"][1] * len(val))
    assert out["fused"][2] == fmt.evaluation_message(out["fused"][1], len(val), 0, out["fused"][0], n_correct)
