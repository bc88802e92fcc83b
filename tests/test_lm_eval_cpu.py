"""Char-LM held-out evaluation on the CPU: ``CharLM.score``,
``LMTrainer.evaluate``, per-epoch validation with a best checkpoint, and the
``lm_cli ... evaluate`` command on checkpoints the CLI trained itself."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_rnn_amd import lm_cli
from pytorch_distributed_rnn_amd.data.charlm import CharCorpus
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import head_nll as hn
from pytorch_distributed_rnn_amd.train.lm import LMTrainer

TINY = ["--vocab", "128", "--embed", "16", "--hidden", "32", "--layers", "2", "--seq-len", "16", "--batch-size", "4",
        "--synthetic-tokens", "4000", "--max-steps", "3", "--device", "cpu", "--dtype", "fp32", "--log", "WARNING"]


def _model(seed=0):
    torch.manual_seed(seed)
    return CharLM(40, 8, 16, 2, compute_dtype=torch.float32)


def _tokens(n, V=40, seed=1):
    return torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(seed))


def test_head_nll_reference_path():
    g = torch.Generator().manual_seed(0)
    h, w, b = torch.randn(3, 5, 16, generator=g), torch.randn(9, 16, generator=g), torch.randn(9, generator=g)
    labels = torch.randint(0, 9, (3, 5), generator=g)
    labels[0, 1] = -100
    labels[2, 2] = 11  # outside the vocabulary: not valid
    assert not hn.supported(16, 9, torch.float32, "cpu")
    accum = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    nll, pred, acc = hn.head_nll(h, w, b, labels, accum=accum)
    logits = F.linear(h.reshape(-1, 16), w, b)
    valid = (labels.reshape(-1) >= 0) & (labels.reshape(-1) < 9)
    ref = F.cross_entropy(logits[valid], labels.reshape(-1)[valid], reduction="none")
    assert torch.allclose(nll[valid], ref, atol=1e-6) and bool((nll[~valid] == 0).all())
    assert torch.equal(pred.long(), logits.argmax(-1)) and pred.dtype == torch.int32
    assert acc is accum and float(acc[1]) == 2.0 + 13 and float(acc[0]) == pytest.approx(1.0 + float(ref.double().sum()))
    assert float(acc[2]) == 3.0 + float((logits.argmax(-1) == labels.reshape(-1))[valid].sum())


def test_score_equals_cross_entropy_and_leaves_the_model_alone():
    model = _model()
    model.train()
    inp, tgt = _tokens(4 * 12).view(4, 12), _tokens(4 * 12, seed=2).view(4, 12)
    with torch.no_grad():
        model(inp[:, :3], carry=True)  # a TBPTT carry to preserve
    kept = model._state
    before = {k: v.clone() for k, v in model.state_dict().items()}
    logprob, pred = model.score(inp, tgt)
    assert model.training and model._state is kept
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    with torch.no_grad():
        logits = model(inp).float()  # [T, B, V]
    ref = -F.cross_entropy(logits.permute(1, 2, 0), tgt, reduction="none")
    assert logprob.shape == (4, 12) and logprob.dtype == torch.float32
    assert torch.allclose(logprob, ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(pred.long(), logits.argmax(-1).t())
    # a continuation: the second half from the first half's state is the whole
    lp1, _, st = model.score(inp[:, :5], tgt[:, :5], return_state=True)
    lp2, _ = model.score(inp[:, 5:], tgt[:, 5:], state=st)
    assert torch.allclose(torch.cat([lp1, lp2], 1), logprob, atol=1e-5, rtol=1e-5)
    ig = tgt.clone()
    ig[1, 3] = -100
    assert float(model.score(inp, ig)[0][1, 3]) == 0.0
    with pytest.raises(ValueError):
        model.score(inp, tgt[:, :-1])


def test_evaluate_is_independent_of_the_window_length():
    model = _model()
    train, held = CharCorpus(_tokens(600), 40), CharCorpus(_tokens(4 * 131 + 3, seed=3), 40)
    tr = LMTrainer(model, train, 4, 16, device=torch.device("cpu"), log_interval=0)
    model.train()
    with torch.no_grad():
        model(train.tokens[:8].view(2, 4), carry=True)
    kept = model._state
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = tr.evaluate(held, 4, 16)
    b = tr.evaluate(held, 4, 64)
    c = tr.evaluate(held, 4)  # the training length
    assert model.training and model._state is kept
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert set(a) == {"loss", "bpc", "accuracy", "tokens", "duration", "tokens_per_sec"}
    assert a["tokens"] == b["tokens"] == 4 * 130  # every target of every stream, the short last window included
    assert a["loss"] == pytest.approx(b["loss"], rel=1e-5) and c["loss"] == a["loss"]
    assert a["accuracy"] == pytest.approx(b["accuracy"], abs=1.5 / a["tokens"])
    assert a["bpc"] == pytest.approx(a["loss"] / math.log(2))
    # against one pass over whole streams
    s = held.streams(4)
    lp, pred = model.score(s[:, :-1], s[:, 1:])
    assert a["loss"] == pytest.approx(float(-lp.double().mean()), rel=1e-5)
    with pytest.raises(ValueError):
        tr.evaluate(CharCorpus(_tokens(5), 40), 4)


def test_train_epoch_validation_keys():
    held = CharCorpus(_tokens(300, seed=4), 40)
    plain = LMTrainer(_model(), CharCorpus(_tokens(600), 40), 4, 16, device=torch.device("cpu"), log_interval=0)
    val = LMTrainer(_model(), CharCorpus(_tokens(600), 40), 4, 16, device=torch.device("cpu"), log_interval=0,
                    validation=held, eval_batch=2)
    a, b = plain.train_epoch(0, 2), val.train_epoch(0, 2)
    assert set(b) - set(a) == {"val_loss", "val_bpc", "val_accuracy"} and a["loss"] == b["loss"]
    assert b["val_loss"] == val.evaluate(held, 2)["loss"]
    assert torch.equal(plain.streams, val.streams)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The tiny model trained through the CLI for two epochs with a held-out
    tenth, and for one epoch without."""
    d, e = tmp_path_factory.mktemp("val"), tmp_path_factory.mktemp("plain")
    hv = lm_cli.main(TINY + ["--epochs", "2", "--validation-fraction", "0.1", "--eval-batch-size", "2",
                             "--checkpoint-directory", str(d), "--history-file", str(d / "history.json"), "local"])
    hp = lm_cli.main(TINY + ["--checkpoint-directory", str(e), "--history-file", str(e / "history.json"), "local"])
    return d, hv, e, hp


def test_cli_validation_history_and_best_checkpoint(runs):
    d, hv, e, hp = runs
    hist = json.loads((d / "history.json").read_text())
    assert len(hist) == 2 and all({"val_loss", "val_bpc", "val_accuracy"} <= set(h) for h in hist)
    assert hist[0]["val_loss"] == hv[0]["val_loss"] and 0 < hist[1]["val_loss"] < math.log(128) + 1
    assert (d / "charlm-best.pt").exists() and (d / "charlm-epoch1.pt").exists()
    # fraction 0: today's keys, no best checkpoint
    plain = json.loads((e / "history.json").read_text())
    assert set(plain[0]) == set(hist[0]) - {"val_loss", "val_bpc", "val_accuracy"}
    assert not (e / "charlm-best.pt").exists()


def test_cli_split_leaves_fraction_zero_alone():
    corpus = CharCorpus.synthetic(4000, 128, seed=0)
    same, none = lm_cli.split_corpus(corpus, 0.0)
    assert same is corpus and none is None
    train, held = lm_cli.split_corpus(corpus, 0.1)
    assert len(held) == 400 and len(train) == 3600
    assert torch.equal(torch.cat([train.tokens, held.tokens]), corpus.tokens)
    assert torch.equal(train.streams(4), corpus.tokens[:3600].view(4, 900))


def test_cli_evaluate_reproduces_the_validation_figure(runs, tmp_path, capsys):
    d, hv, _, _ = runs
    out = tmp_path / "eval.json"
    common = ["--vocab", "128", "--synthetic-tokens", "4000", "--seq-len", "16", "--eval-batch-size", "2", "--device", "cpu",
              "--dtype", "fp32", "--log", "WARNING"]
    res = lm_cli.main(common + ["--checkpoint", str(d / "charlm-epoch1.pt"), "--validation-fraction", "0.1",
                                "--output", str(out), "evaluate"])
    assert res["loss"] == hv[1]["val_loss"] and res["accuracy"] == hv[1]["val_accuracy"]
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("loss ") and " bpc " in line and " accuracy " in line and line.endswith(f"tokens {res['tokens']}")
    saved = json.loads(out.read_text())
    assert saved["loss"] == res["loss"] and saved["tokens"] == res["tokens"] == 2 * 199
    # the best checkpoint is the epoch with the lower validation loss
    best = min(range(2), key=lambda k: hv[k]["val_loss"])
    rb = lm_cli.main(common + ["--checkpoint", str(d / "charlm-best.pt"), "--validation-fraction", "0.1", "evaluate"])
    assert rb["loss"] == hv[best]["val_loss"]
    # without the fraction the whole corpus is scored
    whole = lm_cli.main(common + ["--checkpoint", str(d / "charlm-epoch1.pt"), "evaluate"])
    assert whole["tokens"] == 2 * 1999
    # a text file
    text = tmp_path / "t.txt"
    text.write_bytes(bytes(range(32, 127)) * 3)
    assert lm_cli.main(common + ["--checkpoint", str(d / "charlm-epoch1.pt"), "--text", str(text), "evaluate"])["tokens"] == 2 * 141


def test_cli_evaluate_refusals(runs, tmp_path):
    d = runs[0]
    ck = ["--checkpoint", str(d / "charlm-epoch1.pt"), "--device", "cpu", "--dtype", "fp32", "--log", "WARNING",
          "--vocab", "128", "--synthetic-tokens", "4000"]
    with pytest.raises(SystemExit, match="--checkpoint is required"):
        lm_cli.main(["evaluate"])
    with pytest.raises(SystemExit, match="validation-fraction"):
        lm_cli.main(ck + ["--validation-fraction", "1.0", "evaluate"])
    with pytest.raises(SystemExit, match="eval-batch-size"):
        lm_cli.main(ck + ["--eval-batch-size", "0", "evaluate"])
    with pytest.raises(SystemExit, match="too few"):
        lm_cli.main(ck + ["--validation-fraction", "0.001", "--eval-batch-size", "16", "evaluate"])
    text = tmp_path / "high.txt"
    text.write_bytes(bytes([200, 201, 202, 203] * 20))
    with pytest.raises(SystemExit, match="vocabulary"):
        lm_cli.main(ck + ["--text", str(text), "evaluate"])
    with pytest.raises(SystemExit, match="validation-fraction"):
        lm_cli.main(TINY + ["--validation-fraction", "-0.5", "local"])
