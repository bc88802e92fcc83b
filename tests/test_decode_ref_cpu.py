"""tests/_decode_ref.py against fp64 nn.Embedding + nn.LSTM + nn.Linear stepped
one token at a time, and against the faults it must be able to see."""
import pytest
import torch

import _decode_ref as R

F64 = torch.float64


class _Net(torch.nn.Module):
    def __init__(self, V, E, H, L):
        super().__init__()
        self.embedding = torch.nn.Embedding(V, E)
        self.lstm = torch.nn.LSTM(E, H, L)
        self.fc = torch.nn.Linear(H, V)


def _run(L, defect=None, steps=3):
    """Max |reference - torch| over ``steps`` positions, each reference
    position teacher-forced on torch's state of the position before."""
    torch.manual_seed(3 + L)
    V, E, H, B = 11, 6, 5, 3
    net = _Net(V, E, H, L).double()
    w = R.weights_of(net)
    h = torch.randn(L, B, H, dtype=F64)
    c = torch.randn(L, B, H, dtype=F64)
    worst = 0.0
    with torch.no_grad():
        for p in range(steps):
            tok = torch.randint(0, V, (B,))
            out, (hn, cn) = net.lstm(net.embedding(tok)[None], (h, c))
            logits = net.fc(out[0])
            rh, rc, rl = R.position(w, h, c, tok, defect=defect)
            worst = max(worst, *(float((a - b).abs().max()) for a, b in ((rh, hn), (rc, cn), (rl, logits))))
            h, c = hn, cn
    return worst


@pytest.mark.parametrize("L", [1, 2, 3])
def test_reference_matches_torch_fp64(L):
    assert _run(L) <= 1e-10


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_reference_rejects_planted_defects(defect):
    """Each planted fault moves the reference far outside any bound the GPU
    test grants (1e-2 against 2e-5 + 4e-3 |ref|, |ref| <= 1 for h)."""
    assert _run(2, defect) > 1e-2


def test_weights_rounded_through_the_storage_type():
    torch.manual_seed(0)
    net = _Net(7, 4, 3, 1)
    w = R.weights_of(net, torch.bfloat16)
    assert torch.equal(w["emb"], net.embedding.weight.detach().bfloat16().double())
    assert torch.equal(w["fc_b"], net.fc.bias.detach().double())  # biases stay fp32
    assert R.worst(torch.tensor([1.0 + 2.0 ** -9]), torch.tensor([1.0], dtype=F64), 2.0 ** -8) < 1.0
    assert R.worst(torch.tensor([1.0 + 2.0 ** -7]), torch.tensor([1.0], dtype=F64), 2.0 ** -8) > 1.0
