"""The fused GRU decode kernels (csrc/kernels/lstm_decode.hip, Cell::gru)
through ops/decode.py and ``CharLM(cell="gru")``.

Per position against the fp64 reference of tests/_gru_decode_ref.py, teacher
forced as in test_gpu_decode.py, under _decode_ref.bound = 2e-5 + (1e-4 + r)
|ref| with r half a unit in the last place of the storage relative to the
value: 2^-8 for bf16 h, 2^-11 for fp16 h, 2^-24 for the fp32 master and the
logits.  (2^-9 for bf16 can be met by no kernel: the correctly rounded store of
a value just above 0.5 is off by up to 2^-9 = 2^-8 |ref|.)  Worst |kernel -
ref| / bound measured on an MI355X when this file was written (a correctly
rounded bf16 store alone reaches 0.975); the 11 tests take 3.3 s:

    H, E, L, B        bf16: h     master logits   fp16: h     master logits
    64,  32, 1,  1          0.911 0.007  0.004          0.659 0.006  0.009
    64,  96, 3,  5          0.943 0.031  0.007          0.755 0.039  0.015
    128, 32, 3, 16          0.960 0.020  0.010          0.794 0.022  0.019
    128, 96, 1,  5          0.947 0.019  0.009          0.777 0.026  0.013
"""
import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.ops import decode as dec

import _gru_decode_ref as R

pytestmark = pytest.mark.gpu
ULP_HALF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
V, N = 40, 8
DEV = torch.device("cuda", 0)


def _stack(model):
    return model.embedding.weight, model.gru._weights(), model.fc.weight, model.fc.bias, model.compute_dtype


def _low(model, h0, first, n, **kw):
    return dec.decode(*_stack(model), h0, None, first, n, cell="gru", return_logits=True, **kw)


def _setup(case, cdt):
    H, E, L, B = case
    g = torch.Generator().manual_seed(H + E + B)
    return (R.gru_model(H, E, L, cdt, DEV), (0.5 * torch.randn(L, B, H, generator=g)).to(DEV),
            torch.randint(0, V, (B, N), generator=g).to(DEV), torch.arange(B, device=DEV) % V)


@pytest.mark.parametrize("cdt", list(ULP_HALF), ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "H{}E{}L{}B{}".format(*c))
def test_positions_against_fp64_and_chunking(case, cdt):
    model, h0, forced, first = _setup(case, cdt)
    w = R.weights_of(model, cdt)
    master, h16 = h0, h0.to(cdt)
    worst = {"h": 0.0, "master": 0.0, "logits": 0.0}
    steps = []
    for p in range(N):  # one position per call: every position's entering state is known
        tok, lg, hn, mn = _low(model, master, first, 1, seed=7, pos0=1 + p, forced=forced[:, p:p + 1])
        assert torch.equal(hn, mn.to(cdt))  # the 16-bit h is the master's rounding
        rh, rl = R.position(w, master, forced[:, p], h_own=hn, h_read=h16)
        for name, got, ref, r in (("h", hn, rh, ULP_HALF[cdt]), ("master", mn, rh, 2.0 ** -24), ("logits", lg[:, 0], rl, 2.0 ** -24)):
            worst[name] = max(worst[name], R.worst(got, ref, r))
        steps.append((tok.clone(), lg.clone()))
        master, h16 = mn.clone(), hn.clone()
    print(f"gru decode worst/bound {case} {cdt}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # all N positions in one call: the same bits (the ping-pong's parity), the returned state included
    tok, lg, hn, mn = _low(model, h0, first, N, seed=7, pos0=1, forced=forced)
    assert torch.equal(tok, torch.cat([s[0] for s in steps], 1)) and torch.equal(lg, torch.cat([s[1] for s in steps], 1))
    assert torch.equal(hn, h16) and torch.equal(mn, master)


def test_free_running_equals_forced_and_streams_split():
    model, h0, _, first = _setup((128, 96, 3, 16), torch.bfloat16)
    tok, lg, _, mn = _low(model, h0, first, N, seed=3, pos0=1)
    ft, fl, _, fm = _low(model, h0, first, N, seed=3, pos0=1, forced=torch.cat([first[:, None], tok[:, :-1]], 1))
    assert torch.equal(ft, tok) and torch.equal(fl, lg) and torch.equal(fm, mn)
    for rows in (slice(0, 5), slice(5, 16)):
        t, l, _, m = _low(model, h0[:, rows], first[rows], N, seed=3, pos0=1, stream0=rows.start)
        assert torch.equal(t, tok[rows]) and torch.equal(l, lg[rows]) and torch.equal(m, mn[:, rows])


def test_beam_gathers_the_master_of_the_parent():
    H, E, L, G, W = 64, 32, 2, 2, 4
    model, h0, _, first = _setup((H, E, L, G), torch.bfloat16)
    bufs = dec.alloc_beam_buffers(L, G, W, H, V, N, torch.bfloat16, DEV, return_logits=True)
    hyp, _, _, _, mn = dec.beam_decode(*_stack(model), h0, None, first, N, W, return_logits=True, bufs=bufs, cell="gru")
    parents, at = bufs["parents"].long(), torch.arange(G * W, device=DEV)
    assert bool((parents != at[:, None]).any())  # some beam continues another slot's state
    # the plain path forced to every final hypothesis, each from its prompt's state
    src = at // W
    _, lg, _, fm = _low(model, h0[:, src], first[src], N, temperature=0.0,
                        forced=torch.cat([first[src][:, None], hyp.reshape(G * W, N)[:, :-1]], 1))
    for q in range(N - 1, -1, -1):
        at = parents[at, q]  # the slot each hypothesis held at position q
        assert torch.equal(bufs["logits"][at, q], lg[:, q]), q
    assert torch.equal(mn, fm)
    prompt = torch.tensor([[5, 3], [9, 17]], device=DEV)
    assert torch.equal(model.beam_search(prompt, N, 1)[0][:, 0], model.generate(prompt, N, temperature=0.0))


def test_routing_and_refusals(monkeypatch):
    mod = _ext.require()
    ok = (16, 64, 32, 1024, 2, 0)
    assert mod.gru_decode_supported(*ok) and mod.gru_decode_beam_supported(2, 8, 64, 32, 40, 2, 1)
    for k, bad in ((0, 17), (2, 48), (3, 1025), (5, 2)):  # B = 17, E = 48, V = 1025, fp32
        assert not mod.gru_decode_supported(*ok[:k], bad, *ok[k + 1:])
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    model = R.gru_model(64, 32, 2, torch.bfloat16, DEV, seed=3)
    prompt = torch.tensor([[1, 2], [3, 4]], device=DEV)
    before = model.generate(prompt, 3, temperature=0.0, return_logits=True)[1]
    model.beam_search(prompt, 3, 4)
    model.score(prompt, prompt)
    with pytest.raises(RuntimeError, match="strict"):
        R.gru_model(96, 32, 1, torch.bfloat16, DEV).generate(prompt, 3)
    # the binding reads the padded [4H, .] stacks (the form that measured faster): nn.GRU's own [3H, .] is refused
    stack = list(dec._stack_operands(*_stack(model), "gru"))
    stack[1] = [w[:3 * 64].contiguous() for w in stack[1]]
    bufs = dec.alloc_buffers(2, 2, 64, V, 2, torch.bfloat16, DEV)
    with pytest.raises(RuntimeError, match="4H"):
        mod.gru_decode(*stack, bufs["h"], bufs["c"], bufs["scratch"], prompt[:, -1].contiguous(), None, bufs["tokens"], None, 0.0, 0, 0, 1)
    # in-place updates of the masters reach the 16-bit stacks and the folded bias
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(0.5).add_(0.01)
    after = model.generate(prompt, 3, temperature=0.0, return_logits=True)[1]
    fresh = R.gru_model(64, 32, 2, torch.bfloat16, DEV, seed=4)
    fresh.load_state_dict(model.state_dict())
    assert not torch.equal(after, before) and torch.equal(after, fresh.generate(prompt, 3, temperature=0.0, return_logits=True)[1])
