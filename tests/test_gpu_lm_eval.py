"""Char-LM held-out evaluation on the GPU: ``CharLM.score`` and
``LMTrainer.evaluate`` on the fused head/NLL kernel (the kernel itself:
test_gpu_head_nll.py).  Model: V 96, E 32, H 64, 2 layers, bf16 and fp16, and
the bf16 model again at H 128: at H 64 a bf16 model's recurrence runs on the
small-H kernels, whose output is fp32, so its head takes ops/head_nll.py's
fp32 reference path (announced by a warning); fp16 and bf16 at H 128 run the
16-bit recurrence and the fused kernel."""
import functools
import math

import pytest
import torch

from pytorch_distributed_rnn_amd.data.charlm import CharCorpus
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import head_nll as hn
from pytorch_distributed_rnn_amd.ops.embedding import embedding
from pytorch_distributed_rnn_amd.train.lm import LMTrainer

pytestmark = pytest.mark.gpu

V, E, L = 96, 32, 2
MODELS = [(torch.bfloat16, 64), (torch.float16, 64), (torch.bfloat16, 128)]
IDS = ["bf16", "fp16", "bf16-H128"]
ULP_HALF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _dev():
    return torch.device("cuda", 0)


def _model(cfg, seed=0):
    torch.manual_seed(seed)
    return CharLM(V, E, cfg[1], L, compute_dtype=cfg[0]).to(_dev())


def _fused(cfg):
    """The configuration's top-layer output is 16-bit: the fused kernel runs."""
    return cfg != MODELS[0]


@functools.lru_cache(maxsize=None)
def _tokens(n, seed=1):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


def _stack_output(model, inp, state=None):
    """The top layer's output [T, B, H] as ``score`` computes it."""
    model.eval()
    with torch.no_grad():
        x = embedding(inp.t(), model.embedding.weight, out_dtype=model.compute_dtype)
        out, _ = model.lstm(x, state)
    return out


@pytest.mark.parametrize("cfg", MODELS, ids=IDS)
def test_score_is_head_nll_of_the_stack_output(cfg):
    model = _model(cfg)
    B, T = 5, 23
    inp, tgt = _tokens(B * T).view(B, T).to(_dev()), _tokens(B * T, 2).view(B, T).to(_dev())
    tgt[2, 7] = -100
    model.train()
    with torch.no_grad():
        model(inp[:, :4], carry=True)
    kept = model._state
    logprob, pred = model.score(inp, tgt)
    assert model.training and model._state is kept
    out = _stack_output(model, inp)
    assert hn.supported(cfg[1], V, out.dtype, _dev()) == _fused(cfg) and (out.dtype == cfg[0]) == _fused(cfg)
    nll, p, acc = hn.head_nll(out, model.fc.weight, model.fc.bias, tgt.t().contiguous())
    assert torch.equal(logprob, -nll.view(T, B).t()) and torch.equal(pred, p.view(T, B).t())
    assert float(logprob[2, 7]) == 0.0 and float(acc[1]) == B * T - 1
    # the accumulator a caller passes is the kernel's
    mine = hn.new_accum(_dev())
    model.score(inp, tgt, accum=mine)
    assert torch.equal(mine, acc)


@pytest.mark.parametrize("cfg", MODELS, ids=IDS)
def test_score_agrees_with_forward_to_the_logits_rounding(cfg):
    model, cdt = _model(cfg), cfg[0]
    with torch.no_grad():
        model.fc.weight.mul_(6.0)  # logits of a few units: the 16-bit rounding is what differs
    B, T = 4, 40
    inp, tgt = _tokens(B * T, 3).view(B, T).to(_dev()), _tokens(B * T, 4).view(B, T).to(_dev())
    model.eval()
    logprob, _ = model.score(inp, tgt)
    with torch.no_grad():
        logits = model(inp)  # [T, B, V]: rounded to the compute dtype where the head runs in it
    ref = torch.log_softmax(logits.float(), dim=-1).gather(2, tgt.t()[:, :, None])[:, :, 0].t()
    bound = 2 * ULP_HALF[cdt] * float(logits.float().abs().max())
    err = float((logprob - ref).abs().max())
    print(f"\nscore vs forward + log_softmax {cdt} H={cfg[1]}: max |diff| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("cfg", MODELS, ids=IDS)
def test_evaluate_is_the_mean_of_score(cfg):
    model = _model(cfg)
    corpus, held = CharCorpus(_tokens(2000), V), CharCorpus(_tokens(3 * 101 + 2, 5), V)
    tr = LMTrainer(model, corpus, 4, 16, device=_dev(), log_interval=0)
    ev = tr.evaluate(held, 3, 16)
    s = held.streams(3).to(_dev())
    total, correct, state = 0.0, 0, None
    for k in range(0, 100, 16):
        n = min(16, 100 - k)
        lp, pred, state = model.score(s[:, k:k + n], s[:, k + 1:k + 1 + n], state=state, return_state=True)
        total += float(-lp.double().sum())
        correct += int((pred == s[:, k + 1:k + 1 + n]).sum())
    assert ev["tokens"] == 300
    assert ev["loss"] == pytest.approx(total / 300, rel=1e-12)
    assert ev["accuracy"] == correct / 300 and ev["bpc"] == pytest.approx(ev["loss"] / math.log(2))
    assert tr.evaluate(held, 3, 16)["loss"] == ev["loss"]  # (and again, bit for bit)


@pytest.mark.parametrize("cfg", MODELS, ids=IDS)
def test_training_step_is_unchanged_by_an_evaluation(cfg):
    corpus, held = CharCorpus(_tokens(4 * 200), V), CharCorpus(_tokens(400, 6), V)

    def run(evaluate):
        tr = LMTrainer(_model(cfg), corpus, 4, 16, device=_dev(), log_interval=0)
        tr.inner.train()
        tr.inner.reset_hidden_state()
        segs = list(CharCorpus.segments(tr.streams, 16, 3))
        losses = [tr.train_step(*segs[0]).clone()]
        if evaluate:
            tr.evaluate(held, 2)
            assert tr.inner.training
        losses += [tr.train_step(*segs[1]).clone(), tr.train_step(*segs[2]).clone()]
        tr.settle()
        return torch.stack(losses).cpu()

    a, b = run(False), run(True)
    assert torch.equal(a, b), (a, b)


@pytest.mark.parametrize("cfg", MODELS, ids=IDS)
def test_score_reads_the_updated_head_weight(cfg):
    model = _model(cfg)
    corpus = CharCorpus(_tokens(4 * 200), V)
    tr = LMTrainer(model, corpus, 4, 16, learning_rate=0.05, device=_dev(), log_interval=0)
    B, T = 3, 9
    inp, tgt = _tokens(B * T, 7).view(B, T).to(_dev()), _tokens(B * T, 8).view(B, T).to(_dev())
    before, _ = model.score(inp, tgt)
    model.train()
    tr.train_step(*next(iter(CharCorpus.segments(tr.streams, 16))))
    tr.settle()
    after, _ = model.score(inp, tgt)
    assert not torch.equal(before, after)
    out = _stack_output(model, inp)
    # a clone of the master has no cached 16-bit copy: its cast is made now
    nll, _, _ = hn.head_nll(out, model.fc.weight.detach().clone(), model.fc.bias, tgt.t().contiguous())
    assert torch.equal(after, -nll.view(T, B).t())


def test_evaluate_reruns_after_a_timed_out_persistent_launch():
    """Per-step verification (the multi-rank trainer's mode): a persistent
    recurrence launch flagged as timed out during an evaluation never reaches
    its figures -- the evaluation is run again on the per-step kernels, whose
    result it then equals bit for bit -- and the sticky flag is cleared, so the
    next training step has nothing to re-run."""
    from pytorch_distributed_rnn_amd import _ext
    mod = _ext.require()
    corpus = CharCorpus.synthetic(40_000, seed=3)
    held = CharCorpus(corpus.tokens[-16 * 97 - 5:], 256)
    torch.manual_seed(0)
    tr = LMTrainer(CharLM(256, 64, 1024, 1, compute_dtype=torch.bfloat16), corpus, 16, 32, device=_dev(), log_interval=0)
    seg = next(iter(CharCorpus.segments(tr.streams, 32)))
    try:
        mod.persist_reset()
        mod.set_persist_verify(0)
        mod.persist_disable()  # the per-step kernels' figure
        ref = tr.evaluate(held, 16, 32)
        mod.persist_reset()
        mod.set_persist_verify(2)
        mod.persist_inject_timeouts(1)  # the evaluation's first persistent launch
        got = tr.evaluate(held, 16, 32)
        assert mod.persist_fallbacks() == 1 and mod.persist_disabled()
        assert int(mod.persist_sticky_flag().item()) == 0
        assert got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"] and got["tokens"] == 16 * 96
        tr.inner.train()
        tr.inner.reset_hidden_state()
        loss = tr.train_step(*seg)
        assert tr.settle() == 0 and mod.persist_fallbacks() == 1 and bool(torch.isfinite(loss))
    finally:
        mod.persist_inject_timeouts(0)
        mod.set_persist_verify(0)
        mod.persist_reset()
