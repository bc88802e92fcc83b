"""The ``predict`` subcommand on the CPU: train a tiny model, classify a split
with its checkpoint, and check the JSON and the logged line against the
reloaded model's own forward."""
import json
import subprocess
import sys

import pytest
import torch

from _mp import ROOT, cpu_env, run
from pytorch_distributed_rnn_amd.data.motion import MotionDataset, synthetic_motion
from pytorch_distributed_rnn_amd.models.motion import model_from_state_dict
from pytorch_distributed_rnn_amd.train.checkpoint import read_checkpoint
from pytorch_distributed_rnn_amd.train.formatter import TrainingMessageFormatter

MAIN = ROOT + "/src/motion/main.py"
SEED, N_TRAIN = 3, 96
DATA = ["--seed", str(SEED), "--synthetic", "--synthetic-size", str(N_TRAIN), "--device", "cpu"]
KEYS = {"checkpoint", "split", "examples", "loss", "correct", "accuracy", "class_names", "predictions"}
CELLS = {"lstm": ["--hidden-units", "8"], "gru": ["--hidden-units", "8", "--cell", "gru", "--stacked-layer", "1"]}


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """cell -> (directory, checkpoint) of a one-epoch CPU training run."""
    out = {}
    for cell, flags in CELLS.items():
        d = tmp_path_factory.mktemp(f"predict_{cell}")
        run([sys.executable, MAIN, *DATA, "--epochs", "1", "--batch-size", "48", "--no-validation",
             "--checkpoint-every", "1", "--checkpoint-directory", str(d / "models"), *flags, "local"], cwd=str(d))
        ck = d / "models" / "checkpoint-epoch-1.pt"
        assert ck.exists()
        out[cell] = (d, ck)
    return out


def _split(name):
    return dict(zip(MotionDataset.SPLITS, synthetic_motion(n_train=N_TRAIN, seed=SEED)))[name]


def _check(result, log, ckpt, split):
    """The JSON and the logged line against the reloaded model's forward."""
    assert set(result) == KEYS
    data = _split(split)
    model = model_from_state_dict(read_checkpoint(ckpt)["model_state"]).eval()
    with torch.no_grad():
        logits = model(data.features)
    labels = data.labels.reshape(-1)
    pred = logits.argmax(1)
    assert result["split"] == split and result["checkpoint"] == str(ckpt)
    assert result["examples"] == len(data) == len(result["predictions"])
    assert result["class_names"] == MotionDataset.LABELS
    assert result["predictions"] == pred.tolist()
    assert result["correct"] == int((torch.tensor(result["predictions"]) == labels).sum())
    assert result["accuracy"] == result["correct"] / result["examples"]
    ref_loss = float(torch.nn.functional.cross_entropy(logits.double(), labels))
    # the fp32 mean of n losses summed in any order, plus a few roundings in each loss
    assert abs(result["loss"] - ref_loss) <= (len(data) + 8) * 2.0 ** -24 * max(1.0, ref_loss)
    line = TrainingMessageFormatter(1).evaluation_message(result["accuracy"], result["examples"], None,
                                                          result["loss"], result["correct"])
    assert line.strip() in log


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_train_then_predict(trained, cell):
    d, ck = trained[cell]
    log = run([sys.executable, MAIN, *DATA, *CELLS[cell], "predict", "--checkpoint", str(ck), "--split", "test"],
              cwd=str(d))
    _check(json.load(open(d / "predictions.json")), log, ck, "test")
    assert "ignored" not in log  # the flags given agree with the checkpoint; defaults warn nobody


def test_defaults_do_not_warn(trained):
    """No model flag given: the checkpoint (hidden size 8, one GRU layer)
    differs from every default, and nothing is reported as ignored."""
    d, ck = trained["gru"]
    log = run([sys.executable, MAIN, *DATA, "predict", "--checkpoint", str(ck), "--split", "validation",
               "--predictions-file", "defaults.json"], cwd=str(d))
    assert "ignored" not in log
    _check(json.load(open(d / "defaults.json")), log, ck, "validation")


def test_module_prefix_and_contradicting_flags(trained):
    """A DDP-style checkpoint loads, and the model comes from the checkpoint,
    not from global flags that say otherwise."""
    d, ck = trained["gru"]
    full = read_checkpoint(ck)
    full["model_state"] = {"module." + k: v for k, v in full["model_state"].items()}
    prefixed = d / "models" / "prefixed.pt"
    torch.save(full, prefixed)
    model = model_from_state_dict(full["model_state"])
    assert (model.cell, model.hidden_dim, model.layer_dim, model.bidirectional) == ("gru", 8, 1, False)
    assert model.lstm.input_size == 9 and model.fc.out_features == 6
    log = run([sys.executable, MAIN, *DATA, "--hidden-units", "16", "--stacked-layer", "3", "--cell", "lstm",
               "predict", "--checkpoint", str(prefixed), "--split", "validation",
               "--predictions-file", "prefixed.json"], cwd=str(d))
    assert "--hidden-units 16 ignored" in log and "--cell lstm ignored" in log and "--stacked-layer 3 ignored" in log
    _check(json.load(open(d / "prefixed.json")), log, prefixed, "validation")


def test_predict_needs_a_checkpoint(tmp_path):
    p = subprocess.run([sys.executable, MAIN, *DATA, "predict"], cwd=str(tmp_path), env=cpu_env(),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "--checkpoint" in p.stderr and "required" in p.stderr
