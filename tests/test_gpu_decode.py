"""The fused char-LM decode kernels (csrc/kernels/lstm_decode.hip) through
ops/decode.py and CharLM.generate.

Correctness per position, against the fp64 reference of tests/_decode_ref.py
(proved against fp64 torch modules in test_decode_ref_cpu.py).  The reference
is teacher-forced: every position is evaluated on the state the kernels
themselves stored for the position before, on the forced input token, and --
inside the position -- on the h the kernels stored for the layer below.  Bound,
for every element of every layer's h, of c and of the logits:

    |kernel - ref| <= 2e-5 + (1e-4 + r) |ref|

the bound of tests/test_gpu_lstm_large_steps.py: r is half a unit in the last
place of the stored type, 2^-8 for bf16 h, 2^-11 for fp16 h, 0 for the fp32 c
and logits.  The positions are run one launch sequence at a time (so every
position's h and c can be read back) and again as ONE call, which must give
the same bits: that is what puts the h ping-pong's parity under test.

Every buffer the kernels write sits between two sentinel-filled guard zones
as large as 16 streams' worth of it, which must come back untouched: a store
for a padding stream (batch row >= B) or a vocabulary row >= V would land
there -- or inside a neighbouring layer, slot or row, where the per-element
comparison sees it.

Shapes (H, E, V, layers, B, N):
    64,  32,  24, 1,  1, 1   smallest everything, one position, vocabulary tail
    64,  32,   8, 2,  3, 7   V < 16, odd N (ping-pong parity), cross-layer read
    192, 96,  40, 3, 16, 6   H, E no powers of two, K-split remainder, full batch tile
    128, 64, 256, 2,  5, 4   nonzero initial (h, c), a 3-token prompt through forward

Worst |kernel - ref| / bound measured on an MI355X when this file was written
(a correctly rounded bf16 store alone reaches 2^-8 / (2^-8 + 1e-4) = 0.975):

    shape                      bf16: h     c     logits   fp16: h     c     logits
    64,  32,  24, 1,  1, 1           0.835 0.001 0.000          0.506 0.001 0.000
    64,  32,   8, 2,  3, 7           0.927 0.003 0.000          0.632 0.002 0.000
    192, 96,  40, 3, 16, 6           0.950 0.004 0.000          0.706 0.003 0.000
    128, 64, 256, 2,  5, 4           0.895 0.002 0.000          0.679 0.003 0.001

Device chi-square (7 degrees of freedom, bound 24.32): 3.45 at T = 1, 6.44 at
T = 0.5, the host mirror's figures to the digit.  The 16 cases take 3.3 s.
"""
import functools

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

import _decode_ref as R

pytestmark = pytest.mark.gpu

CASES = [(64, 32, 24, 1, 1, 1), (64, 32, 8, 2, 3, 7), (192, 96, 40, 3, 16, 6), (128, 64, 256, 2, 5, 4)]
DTYPES = [torch.bfloat16, torch.float16]
ULP_HALF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SENTINEL = 12288.0  # exact in bf16, fp16, fp32 and int64
CHI2_999_DF7 = 24.32


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _model(H, E, V, L, cdt, seed=0):
    torch.manual_seed(seed)
    return CharLM(V, E, H, L, compute_dtype=cdt).to(_dev())


def _guarded(shape, dtype):
    """A sentinel-filled flat tensor and the view of its middle that serves as
    the buffer; the guard zones hold 16 leading-dimension rows each."""
    n = 1
    for s in shape:
        n *= s
    inner = n // shape[0] if len(shape) < 4 else shape[-1]  # h [2, L, B, H]: rows of H
    pad = 16 * inner
    flat = torch.full((n + 2 * pad,), SENTINEL, device=_dev(), dtype=dtype)
    return flat, flat[pad:pad + n].view(shape), pad


def _guarded_bufs(L, B, H, V, N, cdt):
    shapes = {"h": ((2, L, B, H), cdt), "c": ((L, B, H), torch.float32), "scratch": ((B, V), torch.float32),
              "tokens": ((B, N), torch.int64), "logits": ((B, N, V), torch.float32)}
    flats, bufs = {}, {}
    for k, (shape, dt) in shapes.items():
        flat, view, pad = _guarded(shape, dt)
        flats[k], bufs[k] = (flat, pad), view
    return flats, bufs


def _assert_guards(flats):
    for k, (flat, pad) in flats.items():
        for zone in (flat[:pad], flat[-pad:]):
            assert bool((zone == SENTINEL).all()), f"{k}: a store outside the buffer"


def _low(model, h0, c0, first, N, bufs=None, **kw):
    return dec.decode(model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias,
                      model.compute_dtype, h0, c0, first, N, bufs=bufs, **kw)


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "H{}E{}V{}L{}B{}N{}".format(*c))
def test_positions_against_fp64(case, cdt):
    H, E, V, L, B, N = case
    model = _model(H, E, V, L, cdt)
    w = R.weights_of(model, cdt)
    g = torch.Generator().manual_seed(H + V + B)
    forced = torch.randint(0, V, (B, N), generator=g).to(_dev())
    prompt, state, P = None, (None, None), 1
    if case == CASES[3]:  # nonzero initial state, then a prompt through forward
        P = 3
        prompt = torch.randint(0, V, (B, P), generator=g).to(_dev())
        state0 = (0.5 * torch.randn(L, B, H, generator=g).to(_dev(), cdt), torch.randn(L, B, H, generator=g).to(_dev(), cdt))
        kept = model._state
        with torch.no_grad():
            model(prompt[:, :-1], state=state0, carry=True)
        state, model._state = model._state, kept
    first = torch.zeros(B, dtype=torch.int64, device=_dev())  # (forced runs never read it)

    # one position per call: every position's h, c and logits against the reference
    h = state[0] if state[0] is not None else torch.zeros(L, B, H, device=_dev(), dtype=cdt)
    c = state[1].float() if state[1] is not None else torch.zeros(L, B, H, device=_dev())
    worst = {"h": 0.0, "c": 0.0, "logits": 0.0}
    steps = []
    for p in range(N):
        flats, bufs = _guarded_bufs(L, B, H, V, 1, cdt)
        tok, lg, hn, cn = _low(model, h, c, first, 1, bufs=bufs, temperature=1.0, seed=11, pos0=P + p,
                               forced=forced[:, p:p + 1], return_logits=True)
        torch.cuda.synchronize()
        _assert_guards(flats)
        rh, rc, rl = R.position(w, h, c, forced[:, p], h_own=hn)
        for name, got, ref, r in (("h", hn, rh, ULP_HALF[cdt]), ("c", cn, rc, 0.0), ("logits", lg[:, 0], rl, 0.0)):
            assert got.shape == ref.shape
            worst[name] = max(worst[name], R.worst(got, ref, r))
        steps.append((tok.clone(), lg.clone()))
        h, c = hn.clone(), cn.clone()
    print(f"decode worst/bound H{H} E{E} V{V} L{L} B{B} N{N} {cdt}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst

    # all N positions in one call: the same bits, nothing outside the buffers
    flats, bufs = _guarded_bufs(L, B, H, V, N, cdt)
    tok, lg, hn, cn = _low(model, state[0], state[1], first, N, bufs=bufs, temperature=1.0, seed=11, pos0=P,
                           forced=forced, return_logits=True)
    torch.cuda.synchronize()
    _assert_guards(flats)
    assert torch.equal(tok, torch.cat([s[0] for s in steps], 1))
    assert torch.equal(lg, torch.cat([s[1] for s in steps], 1))
    assert torch.equal(hn, h) and torch.equal(cn, c)
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    if prompt is not None:  # generate: the prompt through forward, then the same decode
        gt, gl, (gh, gc) = model.generate(prompt, N, temperature=1.0, seed=11, state=state0, forced=forced,
                                          return_logits=True, return_state=True)
        assert torch.equal(gt, tok) and torch.equal(gl, lg) and torch.equal(gh, hn) and torch.equal(gc, cn)


def test_greedy_and_ties():
    H, E, V, L, B, N = 128, 64, 256, 2, 5, 6
    model = _model(H, E, V, L, torch.bfloat16)
    prompt = torch.arange(B * 2).view(B, 2).to(_dev()) % V
    tok, lg = model.generate(prompt, N, temperature=0.0, return_logits=True)
    assert torch.equal(tok, dec.first_argmax(lg))
    # two equal head rows with the largest bias: an exact tie at the top, taken at the lower index
    tied = _model(H, E, V, L, torch.bfloat16, seed=1)
    with torch.no_grad():
        tied.fc.weight[200] = tied.fc.weight[37]
        tied.fc.bias[37] = tied.fc.bias[200] = 3.0
    tok, lg = tied.generate(prompt, N, temperature=0.0, return_logits=True)
    assert torch.equal(lg[..., 37], lg[..., 200])
    assert torch.equal(tok, dec.first_argmax(lg)) and bool((tok == 37).all())


@pytest.mark.parametrize("T", [0.7, 1.0])
def test_sampling_is_the_host_rule(T):
    """tokens = argmax(logits / T + gumbel_noise) computed on the host in fp32
    from the kernels' own logits.  Device and host differ by a few fp32 ulps of
    g <= 17 (the log) and of the quotient, under 1e-5: a draw whose two best
    host values lie within 1e-4 is left out, and at most 1 % may be."""
    H, E, V, L, B, N = 128, 64, 256, 2, 16, 32
    model = _model(H, E, V, L, torch.bfloat16)
    prompt = torch.arange(B).view(B, 1).to(_dev())
    seed = 5
    tok, lg = model.generate(prompt, N, temperature=T, seed=seed, return_logits=True)
    tok, lg = tok.cpu(), lg.cpu()
    streams = torch.arange(B)
    out = 0
    for p in range(N):
        y = lg[:, p] / torch.tensor(T, dtype=torch.float32) + dec.gumbel_noise(seed, streams, 1 + p, V)
        top = y.topk(2, dim=-1).values
        sure = (top[:, 0] - top[:, 1]) >= 1e-4
        out += int((~sure).sum())
        assert torch.equal(tok[sure, p], dec.first_argmax(y)[sure]), p
    assert out <= (B * N) // 100, out


def test_determinism_and_free_running_equals_forced():
    H, E, V, L, B, N = 64, 32, 24, 2, 3, 7
    model = _model(H, E, V, L, torch.float16)
    prompt = torch.tensor([[1, 2], [3, 4], [5, 6]], device=_dev())
    a, la = model.generate(prompt, N, temperature=1.0, seed=3, return_logits=True)
    b, lb = model.generate(prompt, N, temperature=1.0, seed=3, return_logits=True)
    c = model.generate(prompt, N, temperature=1.0, seed=4)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert not torch.equal(a, c)
    forced = torch.cat([prompt[:, -1:], a[:, :-1]], 1)
    f, lf = model.generate(prompt, N, temperature=1.0, seed=3, forced=forced, return_logits=True)
    assert torch.equal(f, a) and torch.equal(lf, la)
    assert model._state is None and model.training  # the carry and the mode are the caller's


def test_batch_independence():
    """A stream's tokens and logits depend on its row index and on nothing
    else in the batch: B = 20 (two groups of 16 and 4), B = 16, B = 1, and row
    17 alone through the op with its global index.  (One-token prompts: no
    batched forward before the decode, whose GEMM plan may depend on B.)"""
    H, E, V, L, N = 128, 64, 256, 2, 5
    model = _model(H, E, V, L, torch.bfloat16)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, V, (20, 1), generator=g).to(_dev())
    h0 = (0.5 * torch.randn(L, 20, H, generator=g)).to(_dev(), torch.bfloat16)
    c0 = torch.randn(L, 20, H, generator=g).to(_dev())
    kw = dict(temperature=1.0, seed=9, return_logits=True)
    t20, l20 = model.generate(prompt, N, state=(h0, c0), **kw)
    t16, l16 = model.generate(prompt[:16], N, state=(h0[:, :16], c0[:, :16]), **kw)
    t1, l1 = model.generate(prompt[:1], N, state=(h0[:, :1], c0[:, :1]), **kw)
    assert torch.equal(t16, t20[:16]) and torch.equal(l16, l20[:16])
    assert torch.equal(t1, t20[:1]) and torch.equal(l1, l20[:1])
    t, l, _, _ = _low(model, h0[:, 17:18], c0[:, 17:18], prompt[17, :], N, stream0=17, pos0=1, **kw)
    assert torch.equal(t, t20[17:18]) and torch.equal(l, l20[17:18])
    assert not torch.equal(t20[16:17], t20[17:18])


def test_distribution_on_the_device():
    """LSTM and head weights zero: the logits are fc.bias = log p exactly, and
    16 x 256 draws must fit softmax(log p / T) (chi-square below the 0.999
    quantile at 7 degrees of freedom; the same seeds pass on the host mirror
    in test_generate_cpu.py)."""
    p = torch.tensor([0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05])
    model = _model(64, 32, 8, 1, torch.bfloat16, seed=2)
    with torch.no_grad():
        for w in model.lstm.parameters():
            w.zero_()
        model.fc.weight.zero_()
        model.fc.bias.copy_(p.log())
    prompt = torch.zeros(16, 1, dtype=torch.int64, device=_dev())
    for T, seed in ((1.0, 0), (0.5, 0)):
        tok = model.generate(prompt, 256, temperature=T, seed=seed).cpu()
        cnt = torch.bincount(tok.flatten(), minlength=8).double()
        e = torch.softmax(p.double().log() / T, 0) * tok.numel()
        chi2 = float(((cnt - e) ** 2 / e).sum())
        print(f"decode chi-square T={T}: {chi2:.2f}")
        assert chi2 < CHI2_999_DF7, (T, chi2)


def test_refusals_and_routing(monkeypatch):
    mod = _ext.require()
    ok = (16, 64, 32, 1024, 2, 0)
    assert mod.lstm_decode_supported(*ok) and mod.lstm_decode_supported(1, 1024, 256, 256, 5, 1)
    for k, bad in ((0, 17), (1, 96), (2, 24), (3, 1025), (5, 2)):
        args = list(ok)
        args[k] = bad
        assert not mod.lstm_decode_supported(*args), args

    calls = []
    real = dec.decode
    monkeypatch.setattr(dec, "decode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    prompt = torch.tensor([[2], [4]], device=_dev())  # (one token: no forward before the decode)
    # fp32: no decode kernel -> the reference path (a warning), an error in strict mode
    torch.manual_seed(0)
    f32 = CharLM(16, 16, 32, 2, compute_dtype=torch.float32).to(_dev())
    with pytest.warns(RuntimeWarning, match="char-LM decode"):
        tok = f32.generate(prompt, 4, temperature=1.0, seed=1)
    assert not calls and tok.shape == (2, 4)
    ref = dec.reference(f32._step, None, prompt[:, -1], 4, temperature=1.0, seed=1, pos0=1)[0]
    f32._state = None
    assert torch.equal(tok, ref)
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    with pytest.raises(RuntimeError, match="strict"):
        f32.generate(prompt, 4)
    # a covered shape: the kernels in strict mode, the reference path when torch kernels are asked for
    model = _model(64, 32, 24, 1, torch.float16)
    fused = model.generate(prompt, 4, temperature=0.0)
    assert calls == [1]
    monkeypatch.setenv("PDRNN_KERNELS", "torch")
    with torch.backends.cudnn.flags(enabled=False):
        slow, ls = model.generate(prompt, 4, temperature=0.0, forced=torch.cat([prompt[:, -1:], fused[:, :-1]], 1),
                                  return_logits=True)
    assert calls == [1] and slow.shape == (2, 4)
    assert torch.equal(slow, dec.first_argmax(ls))


def test_generate_reads_updated_weights():
    """In-place updates of the masters (an optimizer step) reach the 16-bit
    copies the kernels read: the same bits as a fresh model with those weights."""
    H, E, V, L = 64, 32, 24, 2
    model = _model(H, E, V, L, torch.bfloat16, seed=3)
    prompt = torch.tensor([[1, 2], [3, 4]], device=_dev())
    before = model.generate(prompt, 3, temperature=0.0, return_logits=True)[1]
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(0.5).add_(0.01)
    after = model.generate(prompt, 3, temperature=0.0, return_logits=True)[1]
    fresh = CharLM(V, E, H, L, compute_dtype=torch.bfloat16).to(_dev())
    fresh.load_state_dict(model.state_dict())
    want = fresh.generate(prompt, 3, temperature=0.0, return_logits=True)[1]
    assert not torch.equal(after, before)
    assert torch.equal(after, want)
