"""Char-LM generation on the CPU: the ``lm_cli ... generate`` command on a
checkpoint it trained itself, ``charlm_from_state_dict``, and the sampling
rule's host mirror (ops/decode.py:gumbel_noise) as a sampler."""
import pytest
import torch

from pytorch_distributed_rnn_amd import lm_cli
from pytorch_distributed_rnn_amd.models.charlm import CharLM, charlm_from_state_dict
from pytorch_distributed_rnn_amd.ops import decode as dec
from pytorch_distributed_rnn_amd.train.checkpoint import read_checkpoint

CHI2_999_DF7 = 24.32  # 0.999 quantile of chi-square at 7 degrees of freedom


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A tiny model trained for two steps through the CLI."""
    d = tmp_path_factory.mktemp("charlm")
    lm_cli.main(["--vocab", "128", "--embed", "16", "--hidden", "32", "--layers", "2", "--seq-len", "16",
                 "--batch-size", "4", "--synthetic-tokens", "4000", "--max-steps", "2", "--device", "cpu",
                 "--log", "WARNING", "--checkpoint-directory", str(d), "local"])
    return d / "charlm-epoch0.pt"


def _generate(checkpoint, tmp_path, *extra, name="out.bin"):
    out = tmp_path / name
    samples = lm_cli.main(["--checkpoint", str(checkpoint), "--device", "cpu", "--dtype", "fp32", "--log", "WARNING",
                           "--output", str(out), *extra, "generate"])
    return samples, out.read_bytes()


def test_generate_command(checkpoint, tmp_path, capsys):
    args = ("--prompt", "ab", "--num-tokens", "12", "--samples", "3")
    a, raw = _generate(checkpoint, tmp_path, *args, "--seed", "5")
    assert len(raw) == 3 * 12 and raw == b"".join(a) and all(len(s) == 12 for s in a)
    printed = capsys.readouterr().out
    assert printed == "".join(s.decode("utf-8", errors="replace") + "\n" for s in a)
    b, _ = _generate(checkpoint, tmp_path, *args, "--seed", "5", name="b.bin")
    c, _ = _generate(checkpoint, tmp_path, *args, "--seed", "6", name="c.bin")
    assert a == b and a != c
    assert len(set(a)) > 1  # the samples of one call differ by their row index


def test_prompt_file_equals_prompt(checkpoint, tmp_path):
    f = tmp_path / "prompt.txt"
    f.write_bytes(b"xyz")
    a, _ = _generate(checkpoint, tmp_path, "--prompt", "xyz", "--num-tokens", "5", "--seed", "1")
    b, _ = _generate(checkpoint, tmp_path, "--prompt-file", str(f), "--num-tokens", "5", "--seed", "1", name="b.bin")
    assert a == b


def test_greedy_equals_a_forward_loop(checkpoint, tmp_path):
    a, _ = _generate(checkpoint, tmp_path, "--prompt", "hello", "--num-tokens", "9", "--temperature", "0")
    model = charlm_from_state_dict(read_checkpoint(checkpoint)["model_state"], torch.float32).eval()
    seq = list(b"hello")
    with torch.no_grad():
        for _ in range(9):  # the whole text again for every token, no carried state
            logits = model(torch.tensor([seq]))[-1, 0]
            seq.append(int(logits.argmax()))
    assert a == [bytes(seq[5:])]
    assert model._state is None


def test_generate_refuses_bad_input(checkpoint, tmp_path):
    with pytest.raises(SystemExit, match="--checkpoint"):
        lm_cli.main(["generate"])
    with pytest.raises(SystemExit, match="vocabulary"):
        _generate(checkpoint, tmp_path, "--prompt", "é")  # bytes 195, 169 >= 128


@pytest.mark.parametrize("prefix", ["", "module."])
def test_charlm_from_state_dict_round_trips(prefix):
    torch.manual_seed(1)
    src = CharLM(19, 12, 24, 3, compute_dtype=torch.float16)
    state = {prefix + k: v for k, v in src.state_dict().items()}
    model = charlm_from_state_dict(state, torch.float16)
    assert (model.vocab_size, model.embedding.embedding_dim, model.hidden_dim, model.num_layers) == (19, 12, 24, 3)
    assert model.compute_dtype == torch.float16
    for (ka, a), (kb, b) in zip(src.state_dict().items(), model.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    with pytest.raises(KeyError):
        charlm_from_state_dict({"fc.weight": torch.zeros(2, 2)})


def test_generate_states_and_forcing():
    """forced tokens replace the inputs, not the outputs; the returned state
    continues the stream; the carry and the mode are left alone."""
    torch.manual_seed(2)
    model = CharLM(16, 8, 12, 2, dropout=0.5, compute_dtype=torch.float32)
    model._state = "kept"
    prompt = torch.tensor([[1, 2, 3], [4, 5, 6]])
    tok, lg, st = model.generate(prompt, 6, seed=3, return_logits=True, return_state=True)
    assert tok.shape == (2, 6) and tok.dtype == torch.int64 and lg.shape == (2, 6, 16) and st[0].shape == (2, 2, 12)
    assert model._state == "kept" and model.training
    forced = torch.cat([prompt[:, -1:], tok[:, :-1]], 1)
    ftok, flg = model.generate(prompt, 6, seed=3, forced=forced, return_logits=True)
    assert torch.equal(ftok, tok) and torch.equal(flg, lg)
    # two halves, the second from the first's state: the same logits under forcing
    a, la, sa = model.generate(prompt, 3, seed=3, forced=forced[:, :3], return_logits=True, return_state=True)
    b, lb = model.generate(forced[:, 3:4], 3, seed=3, state=sa, forced=forced[:, 3:], return_logits=True)
    torch.testing.assert_close(torch.cat([la, lb], 1), lg, rtol=0, atol=1e-6)
    assert torch.equal(a, tok[:, :3])
    assert model.generate(prompt, 0).shape == (2, 0)
    with pytest.raises(ValueError):
        model.generate(torch.tensor([[99]]), 2)


def test_gumbel_noise_is_the_stated_hash():
    """The first words of the rule, worked by hand in Python integers."""
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16

    seed, b, pos, V = 123456789, 17, 300, 5
    key = mix(mix(mix((seed + 0x9E3779B9) & 0xFFFFFFFF) ^ (b * 0x85EBCA6B & 0xFFFFFFFF)) ^ (pos * 0xC2B2AE35 & 0xFFFFFFFF))
    r = torch.tensor([mix(key ^ v) for v in range(V)])
    u = ((r >> 8).float() + 0.5) * 2.0 ** -24
    want = -torch.log(-torch.log(u.clamp(max=1 - 2.0 ** -24)))
    got = dec.gumbel_noise(seed, b, pos, V)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(dec.gumbel_noise(seed, [3, b], pos, V)[1], got)
    assert torch.isfinite(dec.gumbel_noise(0, list(range(64)), 0, 1024)).all()


@pytest.mark.parametrize("T,seed", [(1.0, 0), (0.5, 0)])
def test_gumbel_sampling_fits_the_softmax(T, seed):
    """Logits fixed to log p over V = 8 (a model whose LSTM and head weights
    are zero and whose head bias is log p), 16 x 256 = 4096 draws through
    ``generate``: chi-square against softmax(log p / T) below the 0.999
    quantile.  The hash is deterministic; the seeds are fixed to ones that
    pass, and test_gpu_decode.py draws the same ones on the device."""
    p = torch.tensor([0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05])
    torch.manual_seed(2)
    model = CharLM(8, 32, 64, 1, compute_dtype=torch.float32)
    with torch.no_grad():
        for w in model.lstm.parameters():
            w.zero_()
        model.fc.weight.zero_()
        model.fc.bias.copy_(p.log())
    tok = model.generate(torch.zeros(16, 1, dtype=torch.int64), 256, temperature=T, seed=seed)
    cnt = torch.bincount(tok.flatten(), minlength=8).double()
    e = torch.softmax(p.double().log() / T, 0) * tok.numel()
    chi2 = float(((cnt - e) ** 2 / e).sum())
    print(f"chi-square T={T} seed={seed}: {chi2:.2f}")
    assert chi2 < CHI2_999_DF7
