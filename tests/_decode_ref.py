"""fp64, teacher-forced reference of ONE char-LM decode position.

``position`` takes the state entering the position exactly as the decode
kernels stored it (h in 16 bits, c in fp32), the input tokens and the weights
as the kernels read them (16-bit-rounded matrices, fp32 biases, all widened to
fp64) and returns every layer's h and c and the logits.  Kernel and reference
so see identical inputs at every position; what is left to differ is the
position's own fp32 arithmetic and the rounding of the h it stores.

The function is plain nn.Embedding + nn.LSTM + nn.Linear semantics (gate order
i, f, g, o) and is proved against those modules in fp64 by
test_decode_ref_cpu.py, which also plants each ``defect`` below and shows the
comparison rejecting it.
"""
import torch

F64 = torch.float64

DEFECTS = ("swap_gates", "stale_lower", "no_c", "no_bias")


def weights_of(model, dtype=None):
    """The fp64 weights of a CharLM-shaped module (``embedding``, ``lstm``,
    ``fc``): matrices rounded through ``dtype`` first (None: as they are),
    biases as stored."""
    def mat(w):
        w = w.detach().cpu()
        return (w.to(dtype) if dtype is not None else w).to(F64)

    def vec(b):
        return b.detach().cpu().to(F64)

    L = model.lstm.num_layers
    return {
        "emb": mat(model.embedding.weight),
        "w_ih": [mat(getattr(model.lstm, f"weight_ih_l{l}")) for l in range(L)],
        "w_hh": [mat(getattr(model.lstm, f"weight_hh_l{l}")) for l in range(L)],
        "b_ih": [vec(getattr(model.lstm, f"bias_ih_l{l}")) for l in range(L)],
        "b_hh": [vec(getattr(model.lstm, f"bias_hh_l{l}")) for l in range(L)],
        "fc_w": mat(model.fc.weight),
        "fc_b": vec(model.fc.bias),
    }


def position(w, h_prev, c_prev, tokens, defect=None, h_own=None):
    """One position.  h_prev / c_prev [L, B, H] (any dtype, widened exactly),
    tokens [B] -> (h [L, B, H], c [L, B, H], logits [B, V]) in fp64.

    ``h_own`` [L, B, H]: the h the kernel stored for THIS position.  Layer
    l > 0 and the head then read the kernel's rounded h of the layer below, as
    the kernel's own launches did, instead of the reference's unrounded one
    (teacher forcing inside the position as well as between positions).

    ``defect`` plants one fault a decode kernel could have: gates f and g
    swapped; layers above 0 fed the PREVIOUS position's h of the layer below;
    c not carried (taken as zero); the biases dropped."""
    assert defect is None or defect in DEFECTS
    h_prev, c_prev = h_prev.detach().cpu().to(F64), c_prev.detach().cpu().to(F64)
    h_own = h_own.detach().cpu().to(F64) if h_own is not None else None
    L = h_prev.shape[0]
    x = w["emb"][tokens.cpu()]
    hs, cs = [], []
    for l in range(L):
        z = x @ w["w_ih"][l].t() + h_prev[l] @ w["w_hh"][l].t()
        if defect != "no_bias":
            z = z + w["b_ih"][l] + w["b_hh"][l]
        i, f, g, o = z.chunk(4, dim=-1)
        if defect == "swap_gates":
            f, g = g, f
        c_in = torch.zeros_like(c_prev[l]) if defect == "no_c" else c_prev[l]
        c = torch.sigmoid(f) * c_in + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        x = h_prev[l] if defect == "stale_lower" else h if h_own is None else h_own[l]
    logits = (hs[-1] if h_own is None else h_own[-1]) @ w["fc_w"].t()
    if defect != "no_bias":
        logits = logits + w["fc_b"]
    return torch.stack(hs), torch.stack(cs), logits


def bound(ref, r):
    """The project's per-element bound (tests/test_gpu_lstm_large_steps.py):
    2e-5 + (1e-4 + r) |ref|, r half a unit in the last place of the storage."""
    return 2e-5 + (1e-4 + r) * ref.abs()


def worst(got, ref, r):
    """max |got - ref| / bound, as a float."""
    return float(((got.detach().cpu().to(F64) - ref).abs() / bound(ref, r)).max())
