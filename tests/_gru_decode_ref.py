"""fp64, teacher-forced reference of ONE GRU char-LM decode position: the GRU
counterpart of tests/_decode_ref.py (whose ``bound`` / ``worst`` it shares),
proved against nn.Embedding + nn.GRU + nn.Linear by test_charlm_gru_cpu.py."""
import torch

from _decode_ref import F64, bound, worst  # noqa: F401  (the callers' bound)

CASES = [(64, 32, 1, 1), (64, 96, 3, 5), (128, 32, 3, 16), (128, 96, 1, 5)]  # (H, E, L, B) of the GPU cases; V = 40


def gru_model(H, E, L, cdt=torch.float32, device="cpu", V=40, seed=0):
    """A ``CharLM(cell="gru")`` with the recurrent matrices scaled by 6, so that some gates saturate and some
    sit near 0, and the head by 8 (tests/_beam_ref.py:lm_model)."""
    from pytorch_distributed_rnn_amd.models.charlm import CharLM
    torch.manual_seed(seed + H + E + L)
    model = CharLM(V, E, H, L, compute_dtype=cdt, cell="gru")
    with torch.no_grad():
        for name, q in model.gru.named_parameters():
            q.mul_(6.0 if name.startswith("weight") else 1.0)
        model.fc.weight.mul_(8.0)
    return model.to(device)


def weights_of(model, dtype=None):
    """The weights as the kernels read them, in fp64: matrices rounded through ``dtype``, biases as stored."""
    def get(name, mat):
        w = name.detach().cpu()
        return (w.to(dtype) if mat and dtype is not None else w).to(F64)

    per = {k: [get(getattr(model.gru, f"{k}_l{l}"), k[0] == "w") for l in range(model.gru.num_layers)]
           for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    return {"emb": get(model.embedding.weight, True), "fc_w": get(model.fc.weight, True), "fc_b": get(model.fc.bias, False), **per}


def position(w, h_prev, tokens, h_own=None, h_read=None, dt=F64):
    """One position evaluated in ``dt``: h_prev [L, B, H] the fp32 master entering it, ``h_read`` the 16-bit h the
    products read (None: h_prev), tokens [B] -> (h [L, B, H], logits [B, V]).  ``h_own``: the 16-bit h the kernel
    stored for THIS position, which the layer above and the head then read (as _decode_ref.position)."""
    w = {k: [m.to(dt) for m in v] if isinstance(v, list) else v.to(dt) for k, v in w.items()}
    h_prev = h_prev.detach().cpu().to(dt)
    h_read = h_read.detach().cpu().to(dt) if h_read is not None else h_prev
    x = w["emb"][tokens.cpu()]
    hs = []
    for l in range(h_prev.shape[0]):
        xr, xz, xn = (x @ w["weight_ih"][l].t() + w["bias_ih"][l]).chunk(3, dim=-1)
        hr, hz, hn = (h_read[l] @ w["weight_hh"][l].t() + w["bias_hh"][l]).chunk(3, dim=-1)
        z, n = torch.sigmoid(xz + hz), torch.tanh(xn + torch.sigmoid(xr + hr) * hn)
        hs.append(n + z * (h_prev[l] - n))
        x = hs[-1] if h_own is None else h_own[l].detach().cpu().to(dt)
    return torch.stack(hs), x @ w["fc_w"].t() + w["fc_b"]
