"""The GRU char-LM on the CPU: the fp64 decode reference against torch's
modules and against an fp32 evaluation, and ``CharLM(cell="gru")`` through
the command line, checkpoints and the generation entry points."""
import pytest
import torch
from torch import nn

from pytorch_distributed_rnn_amd import lm_cli
from pytorch_distributed_rnn_amd.models.charlm import CharLM, charlm_from_state_dict
from pytorch_distributed_rnn_amd.train import checkpoint as ckpt

import _gru_decode_ref as R

CPU = ["--device", "cpu", "--dtype", "fp32", "--log", "WARNING"]
DATA = ["--vocab", "128", "--synthetic-tokens", "4000", "--seq-len", "16", "--eval-batch-size", "2", "--validation-fraction", "0.1"]


@pytest.mark.parametrize("L", [1, 2])
def test_reference_is_torch_gru_in_fp64(L):
    V, E, H, B = 11, 8, 16, 3
    torch.manual_seed(L)
    model = CharLM(V, E, H, L, compute_dtype=torch.float32, cell="gru").double()
    gru = nn.GRU(E, H, L).double()
    gru.load_state_dict(model.gru.state_dict())
    w, h = R.weights_of(model), torch.randn(L, B, H, dtype=torch.float64)
    for p in range(4):
        tok = torch.randint(0, V, (B,))
        with torch.no_grad():
            out, want = gru(model.embedding(tok)[None], h)
            want_logits = model.fc(out[0])
        h, logits = R.position(w, h, tok)
        assert float((h - want).abs().max()) <= 1e-12 and float((logits - want_logits).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "H{}E{}L{}B{}".format(*c))
def test_fp32_evaluation_is_well_inside_the_bound(case):
    """The GPU cases' positions in fp32 against fp64, both on bf16-rounded weights."""
    H, E, L, B = case
    w = R.weights_of(R.gru_model(H, E, L), torch.bfloat16)
    g = torch.Generator().manual_seed(H + E + B)
    h = (0.5 * torch.randn(L, B, H, generator=g)).float()
    for p in range(8):
        tok = torch.randint(0, 40, (B,), generator=g)
        (want, logits), (h, lg) = R.position(w, h, tok), R.position(w, h, tok, dt=torch.float32)
        assert R.worst(h, want, 2.0 ** -24) < 0.5 and R.worst(lg, logits, 2.0 ** -24) < 0.5


def test_cli_trains_generates_searches_and_evaluates(tmp_path):
    hist = lm_cli.main(DATA + CPU + ["--embed", "16", "--hidden", "32", "--batch-size", "4", "--max-steps", "3", "--cell", "gru",
                                     "--checkpoint-directory", str(tmp_path), "local"])
    ck = ["--checkpoint", str(tmp_path / "charlm-epoch0.pt")]
    gen = ck + CPU + ["--prompt", "ab", "--num-tokens", "6", "--samples", "2"]
    assert [len(s) for s in lm_cli.main(gen + ["generate"])] == [6, 6]
    assert len(lm_cli.main(gen + ["--beam-width", "3", "generate"])) == 2
    assert lm_cli.main(ck + DATA + CPU + ["evaluate"])["loss"] == hist[0]["val_loss"]
    state = ckpt.read_checkpoint(ck[1])["model_state"]
    model = charlm_from_state_dict(state, torch.float32)
    assert model.cell == "gru" and model.gru.num_layers == 2 and model.hidden_dim == 32 and not hasattr(model, "lstm")
    assert all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    with pytest.raises(ValueError, match="weight_hh_l0"):
        charlm_from_state_dict({k: (v[:64] if k == "gru.weight_hh_l0" else v) for k, v in state.items()}, torch.float32)


def test_lstm_keys_are_unchanged():
    lstm = CharLM(9, 4, 8, 2, compute_dtype=torch.float32)
    names = [f"lstm.{k}_l{l}" for l in range(2) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert lstm.cell == "lstm" and sorted(lstm.state_dict()) == sorted(["embedding.weight", "fc.weight", "fc.bias"] + names)
    assert charlm_from_state_dict(lstm.state_dict(), torch.float32).cell == "lstm"
    with pytest.raises(ValueError, match="cell"):
        CharLM(9, 4, 8, 1, cell="rnn")


def test_gru_state_is_one_tensor_everywhere():
    model = R.gru_model(16, 8, 2)
    prompt, h0 = torch.tensor([[1, 2, 3], [4, 5, 6]]), 0.5 * torch.randn(2, 2, 16)
    tok, h = model.generate(prompt, 5, temperature=0.0, state=h0, return_state=True)
    assert isinstance(h, torch.Tensor) and h.shape == (2, 2, 16) and model._state is None
    assert torch.equal(model.generate(torch.cat([prompt, tok[:, :2]], 1), 3, temperature=0.0, state=h0), tok[:, 2:])
    assert model.beam_search(prompt, 5, 3, length_penalty=0.7, return_state=True)[3].shape == (2, 6, 16)
    assert torch.equal(model.beam_search(prompt, 5, 1, state=h0)[0][:, 0], tok)
    assert model.score(prompt, prompt, state=h0, return_state=True)[2].shape == (2, 2, 16)
