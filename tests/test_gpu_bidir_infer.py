"""GPU: the one-launch bidirectional motion inference kernel
(kernels/lstm_bidir_infer.hip: lstm_bidir_head_infer, lstm_bidir_infer_plan,
lstm_bidir_infer_ok) against torch.nn.LSTM(bidirectional=True) + nn.Linear in
fp64 on the CPU, and its routing through train/fused_eval.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 32
U = 2.0 ** -24
# Per-element logit bound.  The unidirectional test's bound is tied to the
# kernel's own h_n, which this kernel does not return, so: the worst error of
# the same reference run in fp32 on the CPU against fp64 over CASES, the
# gathered and the saturating cases is 3.1e-7 (measured: the two-layer
# saturating case, logits up to 1.5; 4.6e-8 over CASES alone, logits up to
# 0.3); the kernel gets 16 times that for v_exp_f32 / v_rcp_f32 against libm
# through up to 2 x 128 recurrent steps.
TOL = 16 * 3.1e-7

#        T    B   I  L  C   head bias
CASES = [(1, 1, 1, 1, 1, True), (1, 3, 9, 2, 6, True), (2, 2, 9, 2, 6, False), (15, 3, 12, 1, 16, True),
         (16, 17, 9, 2, 6, True), (16, 2, 12, 1, 1, False), (17, 3, 1, 2, 16, False), (33, 17, 12, 2, 1, True),
         (128, 17, 9, 1, 6, False), (128, 3, 9, 2, 6, True)]


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.native(torch.device("cuda", 0))


def _planned(L, B, T):
    """The plan's rule, restated: as many sequences per workgroup as 64 KiB of
    LDS holds (at most 4), fewer while CUs would stay without a workgroup."""
    seq = 4 * (208 + 12 * T + (72 * T + 4352 if L == 2 else 0))
    ns = min(4, 65536 // seq)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    while ns > 1 and -(-B // ns) < cus:
        ns -= 1
    return ns, seq


@functools.lru_cache(maxsize=None)
def _case(T, B, I, L, C, bias, saturate=False):
    """A seeded stack, head and input (fp32 values), the fp64 logits of
    fc(out[:, -1, :]), all on the CPU (_launch copies what the kernel reads)."""
    torch.manual_seed(1000 * T + 100 * B + 10 * I + L + C)
    rnn = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True)
    fc = torch.nn.Linear(2 * H, C, bias=bias)
    if saturate:  # i, f, o within 4e-4 of 1 and g of +-1 (alternating by unit) at every step
        sign = 1.0 - 2.0 * (torch.arange(H) % 2)
        with torch.no_grad():
            for name, p in rnn.named_parameters():
                if name.startswith("bias_ih"):
                    p.view(4, H).add_(8.0 * torch.stack([torch.ones(H), torch.ones(H), sign, torch.ones(H)]))
    x = torch.randn(B, T, I)
    with torch.no_grad():
        ref = fc.double()(rnn.double()(x.double())[0][:, -1, :])
    ws = [p.detach().float() for p in rnn.parameters()]
    return rnn, fc, x, ref, ws, fc.weight.detach().float(), (fc.bias.detach().float() if bias else None)


def _guarded(shape, dtype):
    n = int(torch.tensor(shape).prod())
    flat = torch.full((n + 128,), 777, device="cuda", dtype=dtype)
    return flat, flat[64:64 + n].view(shape)


def _launch(x, ws, hw, hb, L, ns=-1, labels=None, idx=None):
    """One launch: x inside NaN padding (unless gathered), the outputs between
    sentinel guard zones, the plan's choice asserted first."""
    ws, hw, hb, x = [w.cuda() for w in ws], hw.cuda(), (None if hb is None else hb.cuda()), x.cuda()
    B, T = (idx.numel() if idx is not None else x.shape[0]), x.shape[1]
    want_ns, want_lds = _planned(L, B, T)
    plan = _mod().lstm_bidir_infer_plan(L, B, T)
    assert (plan["ns"], plan["lds"]) == (want_ns, want_ns * want_lds)
    if idx is None:
        pad = torch.full((B + 2, T + 2, x.shape[2] + 3), float("nan"), device="cuda")
        pad[1:-1, 1:-1, 1:-2] = x
        x = pad[1:-1, 1:-1, 1:-2]
    C = hw.shape[0]
    (fl, lo), (fp, pr), (fs, st) = _guarded((B, C), torch.float32), _guarded((B,), torch.int64), _guarded((B, 3), torch.float32)
    out = _mod().lstm_bidir_head_infer(x, idx, labels, ws, hw, hb, H, L, ns=ns, logits_out=lo, pred_out=pr, stats_out=st)
    torch.cuda.synchronize()
    for flat in (fl, fp, fs):
        assert bool((flat[:64] == 777).all()) and bool((flat[-64:] == 777).all()), "a store outside an output"
    assert out[0].data_ptr() == lo.data_ptr() and (labels is None) == (out[2] is None)
    return out[0].clone(), out[1].clone(), (None if labels is None else out[2].clone())


def _check(logits, pred, stats, ref, labels, what):
    err = (logits.double().cpu() - ref).abs().max().item()
    print(f"{what}: max |logit - fp64| {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL, what
    top = ref.topk(2, dim=1).values if ref.shape[1] > 1 else None
    clear = torch.ones(len(ref), dtype=torch.bool) if top is None else (top[:, 0] - top[:, 1]) > 2 * TOL
    assert torch.equal(pred.cpu()[clear], ref.argmax(1)[clear]), what
    if stats is not None:
        B = len(ref)
        loss = torch.nn.functional.cross_entropy(ref, labels.cpu(), reduction="none")
        # log-sum-exp is 1-Lipschitz in the largest logit error and z_y moves by as much: 2 TOL,
        # plus the fp32 roundings of exp / log / the 1 / B scaling at the loss's magnitude
        lerr = ((stats[:, 0].double().cpu() * B) - loss).abs()
        assert bool((lerr <= 2 * TOL + 16 * U * loss.clamp(min=1.0)).all()), (what, lerr.max().item())
        assert torch.equal(stats[:, 1], torch.ones(B, device="cuda"))
        assert torch.equal(stats[:, 2], (pred == labels).float())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{}B{}I{}L{}C{}{}".format(*c[:5], "b" if c[5] else ""))
def test_logits_predictions_statistics_against_fp64(case):
    """Every sequences-per-workgroup count the LDS allows (B = 3 at 2 and B = 17
    at 4: a partly filled last workgroup), with labels; two launches, equal bits."""
    T, B, I, L, C, bias = case
    _, _, x, ref, ws, hw, hb = _case(*case)
    torch.manual_seed(7)
    labels = torch.randint(0, C, (B,), device="cuda")
    for ns in [-1] + [n for n in (1, 2, 4) if n * _planned(L, B, T)[1] <= 65536]:
        got = _launch(x, ws, hw, hb, L, ns=ns, labels=labels)
        _check(*got, ref, labels, f"{case} ns={ns}")
        again = _launch(x, ws, hw, hb, L, ns=ns, labels=labels)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    with pytest.raises(RuntimeError):
        _launch(x, ws, hw, hb, L, ns=5)


def test_gathered_table_and_saturated_gates():
    """x gathered through idx from a larger table (labels through it too); a
    stack whose biases drive every gate to within 4e-4 of 1 or +-1."""
    T, B, I, L, C = 33, 5, 9, 2, 6
    _, _, x, ref, ws, hw, hb = _case(T, 12, I, L, C, True)
    idx = torch.tensor([7, 0, 11, 3, 7], device="cuda")
    labels = torch.arange(12, device="cuda") % C
    lo, pr, st = _launch(x, ws, hw, hb, L, labels=labels, idx=idx)
    _check(lo, pr, st, ref[idx.cpu()], labels[idx], "gathered")
    for L in (1, 2):
        _, _, x, ref, ws, hw, hb = _case(17, 3, 9, L, 6, True, True)
        lo, pr, _ = _launch(x, ws, hw, hb, L)
        _check(lo, pr, None, ref, None, f"saturated L={L}")


@pytest.mark.parametrize("L", [1, 2])
def test_ties_take_the_lowest_class(L):
    _, _, x, _, ws, _, _ = _case(16, 3, 9, L, 6, True)
    hw, hb = torch.zeros(16, 2 * H, device="cuda"), torch.full((16,), 0.25, device="cuda")
    lo, pr, st = _launch(x, ws, hw, hb, L, labels=torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert torch.equal(lo, torch.full((3, 16), 0.25, device="cuda"))
    assert torch.equal(pr, torch.zeros(3, dtype=torch.int64, device="cuda")) and bool((st[:, 2] == 1).all())


@pytest.mark.parametrize("L", [1, 2])
def test_reverse_half_reads_the_last_position_only(L):
    """A head whose forward-half columns are zero sees the top layer's reverse
    state alone.  Changing x[:, :T-1] leaves it bit-identical with one layer
    (one step at x[T-1]) and moves it with two (layer 0's reverse pass feeds it)."""
    _, _, x, _, ws, hw, hb = _case(17, 3, 9, L, 6, True)
    hw = hw.clone()
    hw[:, :H] = 0
    x2 = x.clone()
    x2[:, :-1] += 1.0
    a, b = _launch(x, ws, hw, hb, L)[0], _launch(x2, ws, hw, hb, L)[0]
    assert torch.equal(a, b) if L == 1 else not torch.equal(a, b)
    x3 = x.clone()
    x3[:, -1] += 1.0
    assert not torch.equal(a, _launch(x3, ws, hw, hb, L)[0])


def test_refusals():
    mod = _mod()
    assert mod.lstm_bidir_infer_ok(32, 12, 2, 0) and mod.lstm_bidir_infer_ok(32, 1, 1, 0)
    for bad in ((16, 9, 2, 0), (64, 9, 2, 0), (32, 13, 2, 0), (32, 0, 1, 0), (32, 9, 3, 0), (32, 9, 2, 1)):
        assert not mod.lstm_bidir_infer_ok(*bad), bad
    assert mod.lstm_bidir_infer_plan(2, 3, 140)["ns"] == 1 and mod.lstm_bidir_infer_plan(1, 3, 1348)["ns"] == 1
    for L, T in ((2, 141), (1, 1349)):
        with pytest.raises(RuntimeError):
            mod.lstm_bidir_infer_plan(L, 3, T)
    _, _, x, _, ws, hw, hb = _case(16, 3, 9, 2, 6, True)
    x, ws, hw, hb = x.cuda(), [w.cuda() for w in ws], hw.cuda(), hb.cuda()
    calls = {"C = 17": (x, ws, torch.zeros(17, 2 * H, device="cuda"), None, H, 2),
             "no bias": (x, [w for i, w in enumerate(ws) if i % 4 < 2], hw, hb, H, 2),
             "H = 16": (x, ws, hw, hb, 16, 2), "L = 3": (x, ws + ws[4:], hw, hb, H, 3),
             "I = 13": (torch.zeros(3, 16, 13, device="cuda"), ws, hw, hb, H, 2),
             "T = 141": (torch.zeros(3, 141, 9, device="cuda"), ws, hw, hb, H, 2),
             "head [C, H]": (x, ws, hw[:, :H].contiguous(), hb, H, 2)}
    for what, (xx, w, a, b, h, L) in calls.items():
        with pytest.raises(RuntimeError):
            mod.lstm_bidir_head_infer(xx, None, None, w, a, b, h, L)
            pytest.fail(what)


@pytest.mark.parametrize("L", [1, 2])
def test_routing_predict_evalstep_and_trainer(L, monkeypatch):
    """A bidirectional H = 32 MotionModel takes the kernel: predict, the
    accumulator over two batches plus a refused-T batch, and Trainer._evaluate
    against PDRNN_FUSED_EVAL=0 (both paths lie within TOL of fp64 on O(1)
    logits: 2 TOL between them)."""
    from pytorch_distributed_rnn_amd.data.motion import synthetic_motion
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    from pytorch_distributed_rnn_amd.train import fused_eval
    from pytorch_distributed_rnn_amd.train.formatter import TrainingMessageFormatter
    from pytorch_distributed_rnn_amd.train.trainer import Trainer
    torch.manual_seed(20 + L)
    model = MotionModel(9, H, L, 6, bidirectional=True).cuda().eval()
    dev = torch.device("cuda")
    assert fused_eval.supported(model, dev)
    for attr, val in (("proj_size", 8), ("bias", False)):
        monkeypatch.setattr(model.lstm, attr, val)
        assert not fused_eval.supported(model, dev)
        monkeypatch.undo()
    assert not fused_eval.supported(MotionModel(9, H, L, 6, cell="gru", bidirectional=True).cuda(), dev)
    ref64 = MotionModel(9, H, L, 6, bidirectional=True).double()
    ref64.load_state_dict({k: v.double().cpu() for k, v in model.state_dict().items()})
    xs = [torch.randn(5, 32, 9, device="cuda"), torch.randn(3, 32, 9, device="cuda"), torch.randn(2, 1400 if L == 1 else 160, 9, device="cuda")]  # (the last: refused by the plan)
    ys = [torch.randint(0, 6, (len(x),), device="cuda") for x in xs]
    step = fused_eval.MotionEvalStep(model)
    want_loss, want_correct = 0.0, 0
    for x, y in zip(xs, ys):
        with torch.no_grad():
            ref, old = ref64(x.double().cpu()), model(x)
        logits, pred = step(x, y)
        assert torch.equal(model.predict(x), logits)
        if x.shape[1] == 32:
            assert (logits.double().cpu() - ref).abs().max().item() <= TOL
            assert (logits - old).abs().max().item() <= 2 * TOL
        else:  # model.forward's own result, in the same accumulator
            assert torch.equal(logits, old)
            ref = old.double().cpu()
        assert torch.equal(pred, logits.argmax(1))
        want_loss += torch.nn.functional.cross_entropy(ref, y.cpu()).item()
        want_correct += int((logits.argmax(1) == y).sum())
    loss_sum, n, correct, batches = step.result()
    assert (n, correct, batches) == (10, want_correct, 3)
    assert abs(loss_sum - want_loss) <= 3 * (2 * TOL + 16 * U * max(1.0, want_loss))

    train, val, _ = synthetic_motion(n_train=48, n_validation=100, n_test=2, seq_length=32, seed=91)
    trainer = Trainer(model, train, batch_size=48, learning_rate=2.5e-3, validation_set=val, device=dev, warmup=False)
    loader = trainer._get_data_loader(val, batch_size=40)
    out = {}
    for env in ("1", "0"):
        monkeypatch.setenv("PDRNN_FUSED_EVAL", env)
        out[env] = trainer._evaluate(loader, TrainingMessageFormatter(1), epoch=0)
    top = model.predict(val.features.cuda()).double().topk(2, dim=1).values
    if (top[:, 0] - top[:, 1]).min().item() > 4 * TOL:
        assert out["1"][1] == out["0"][1]
    assert abs(out["1"][0] - out["0"][0]) <= 2 * (2 * TOL + 16 * U * max(1.0, out["0"][0]))
