"""Top-k / nucleus filtering inside the fused char-LM decode kernels
(csrc/kernels/lstm_decode.hip: sample_tokens_filtered), their ``threshold`` and
``logprobs`` outputs, and ``stop``, through ops/decode.py and CharLM.generate.

The rule is pdrnn/decode_rng.h's; its host mirror ops/decode.py:keep_threshold
is proved against a sort-and-walk implementation in test_decode_filter_cpu.py
and is the fp64 yardstick here, always applied to the logits the kernels
themselves returned.

Bounds, with u = 2^-24 (half an fp32 ulp) and Y = max |logit / T| over the
logits of the test (asserted <= 16):

* top-k threshold: exact.  Counts are integers.
* nucleus threshold: the device compares S(tau) >= fl(top_p * S(tau_k)), S a
  sum of w_v = expf(fl(fl(l_v / T) - fl(max / T))).  The exponent's argument
  carries u |y_v| + u |max y| + u |y_v - max y| <= 4 u Y of error, expf itself
  one ulp = 2 u, so each w_v is off by at most (4 Y + 2) u relative; a lane adds
  its <= 16 weights in order (15 u) and the butterfly adds 6 levels (6 u), all
  terms >= 0, so S is off by at most (4 Y + 23) u relative.  Two such sums, the
  fp32 product and top_p's own rounding to fp32 give: the device's test is the
  exact one at some top_p' with |top_p' / top_p - 1| <= d = (8 Y + 48) u
  (1.05e-5 at Y = 16).  tau does not grow with top_p, so the device's threshold
  must be a value of its row with tau64(top_p (1 + d)) <= threshold <=
  tau64(top_p (1 - d)).
* log-prob: lp = fl(fl(fl(l_tok / T) - max y) - logf(S)): 4 u Y from the first
  difference, (4 Y + 23) u from S inside the log, one ulp of logf (2 u log V <=
  14 u at V <= 1024), u |lp| <= (2 Y + 7) u from the last difference:
  |lp - lp64| <= (10 Y + 44) u, 1.22e-5 at Y = 16.

Measured on an MI355X when this file was written: worst log-prob error 0.115
(bf16 model) / 0.107 (fp16) of that bound; d between 5.7e-6 and 7.8e-6, the two
fp64 thresholds of the bracket differing in 0 to 5 of the 128 rows of a
setting; filtered chi-squares 1.95 (top_k 3), 1.33 (top_k 4, five kept), 1.95
(top_p 0.6), the host mirror's figures.  The 41 cases take 4.4 s.
"""
import functools

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

pytestmark = pytest.mark.gpu

F64 = torch.float64
INF = float("inf")
U = 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 12288.0  # exact in bf16, fp16, fp32 and int64
FILTERS = [(40, 1.0), (0, 0.9), (40, 0.9)]
CHI2_999 = {2: 13.816, 4: 18.467}
P8 = [0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _model(H, E, V, L, cdt, seed=0, spread=0.0):
    """spread > 0: a head whose logits spread over a few units (bias
    ~ spread * N(0, 1), weights x 4 so that rows differ by stream and position)."""
    torch.manual_seed(seed)
    model = CharLM(V, E, H, L, compute_dtype=cdt).to(_dev())
    if spread:
        with torch.no_grad():
            model.fc.weight.mul_(4.0)
            model.fc.bias.copy_(torch.randn(V) * spread)
    return model


def _bias_model(V, cdt):
    """LSTM and head weights zero: every stream's logits are fc.bias exactly."""
    model = _model(64, 32, V, 1, cdt, seed=7)
    with torch.no_grad():
        for w in model.lstm.parameters():
            w.zero_()
        model.fc.weight.zero_()
    return model


def _guarded(shape, dtype):
    """A sentinel-filled flat tensor and the view of its middle that serves as
    the buffer; the guard zones hold 16 leading-dimension rows each."""
    n = 1
    for s in shape:
        n *= s
    inner = n // shape[0] if len(shape) < 4 else shape[-1]
    pad = 16 * inner
    flat = torch.full((n + 2 * pad,), SENTINEL, device=_dev(), dtype=dtype)
    return flat, flat[pad:pad + n].view(shape), pad


def _guarded_bufs(L, B, H, V, N, cdt):
    f32 = torch.float32
    shapes = {"h": ((2, L, B, H), cdt), "c": ((L, B, H), f32), "scratch": ((B, V), f32), "tokens": ((B, N), torch.int64),
              "logits": ((B, N, V), f32), "threshold": ((B, N), f32), "logprobs": ((B, N), f32)}
    flats, bufs = {}, {}
    for k, (shape, dt) in shapes.items():
        flat, view, pad = _guarded(shape, dt)
        flats[k], bufs[k] = (flat, pad), view
    return flats, bufs


def _assert_guards(flats):
    for k, (flat, pad) in flats.items():
        for zone in (flat[:pad], flat[-pad:]):
            assert bool((zone == SENTINEL).all()), f"{k}: a store outside the buffer"


def _low(model, first, N, h0=None, c0=None, bufs=None, **kw):
    """The op: (tokens, logits, h, c, threshold, logprobs)."""
    kw = {"return_logits": True, "return_threshold": True, "return_logprobs": True, **kw}
    return dec.decode(model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias,
                      model.compute_dtype, h0, c0, first, N, bufs=bufs, **kw)


def _groups(model, first, N, h0, c0, **kw):
    """B > 16 as generate runs it: independent groups of 16 with stream0 = the
    group's first row -> (tokens, threshold, logprobs), concatenated."""
    outs = []
    for b0 in range(0, first.shape[0], dec.MAX_STREAMS):
        rows = slice(b0, b0 + dec.MAX_STREAMS)
        o = _low(model, first[rows], N, h0[:, rows], c0[:, rows], stream0=b0, **kw)
        outs.append([o[0].clone(), o[4].clone(), o[5].clone()])
    return [torch.cat(x, 0) for x in zip(*outs)]


def _rows(V):
    """Head biases: ties at the k-th value for k = 2, 40 and V - 1; -inf entries;
    a mixed-sign row with an exact zero."""
    g = torch.Generator().manual_seed(V)
    ties = torch.randn(V, generator=g) * 3
    order = ties.argsort(descending=True)
    for k in (2, 40, V - 1):  # the k-th largest shared by its two neighbours in rank
        if 1 < k < V:
            ties[order[k - 2:k + 1]] = float(ties[order[k - 1]])
    holes = torch.randn(V, generator=g) * 3
    holes[torch.randperm(V, generator=g)[:V // 3]] = -INF
    mixed = torch.randn(V, generator=g) * 1e-3
    mixed[V // 2] = 0.0
    mixed[torch.randperm(V, generator=g)[:2]] = torch.tensor([40000.0, -40000.0])
    return {"ties": ties, "holes": holes, "mixed": mixed}


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("V", [8, 24, 64, 65, 256, 300, 512, 1000, 1024])
def test_top_k_threshold_is_exact(V, cdt):
    """threshold == the k-th largest of the kernels' own logits, bit for bit,
    at every position of every stream; -inf where top_k >= V.  All buffers
    between guard zones: padding streams (B < 16) are never written."""
    model = _bias_model(V, cdt)
    N = 8
    for name, bias in _rows(V).items():
        with torch.no_grad():
            model.fc.bias.copy_(bias)
        for B in (1, 5, 16):
            first = torch.arange(B, device=_dev()) % V
            for k in (1, 2, V - 1, 40):
                flats, bufs = _guarded_bufs(1, B, 64, V, N, cdt)
                tok, lg, _, _, thr, lp = _low(model, first, N, bufs=bufs, temperature=1.0, seed=V + k, top_k=k)
                torch.cuda.synchronize()
                _assert_guards(flats)
                assert torch.equal(lg, model.fc.bias.detach().expand(B, N, V)), (name, B, k)
                want = lg.sort(dim=-1, descending=True).values[..., k - 1] if k < V else torch.full_like(thr, -INF)
                assert torch.equal(thr, want), (name, B, k)
                assert int(tok.min()) >= 0 and int(tok.max()) < V
                assert bool((lg.gather(-1, tok[..., None])[..., 0] >= thr).all()), (name, B, k)
                kept = (lg >= thr[..., None]).sum(-1)
                assert bool((kept >= k).all() if k < V else (kept == V).all())
                assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("V", [256, 1000])
def test_nucleus_threshold_is_bracketed(V, T):
    """See the module docstring: the device's threshold is a value of the row
    between the fp64 thresholds at top_p (1 + d) and top_p (1 - d)."""
    B, N = 16, 8
    model = _model(64, 32, V, 1, torch.bfloat16, seed=3, spread=2.0)
    first = torch.arange(B, device=_dev()) % V
    T32 = float(torch.tensor(T, dtype=torch.float32))  # the temperature the kernels divide by
    for k in (0, 40):
        for p in (0.5, 0.9, 0.95):
            tok, lg, _, _, thr, _ = _low(model, first, N, temperature=T, seed=1, top_k=k, top_p=p)
            lg64, thr64 = lg.double().cpu(), thr.double().cpu()
            Y = float(lg64.abs().max()) / T32
            assert Y <= 16
            d = (8 * Y + 48) * U
            lo, hi = dec.keep_threshold(lg64, T32, k, p * (1 + d)), dec.keep_threshold(lg64, T32, k, p * (1 - d))
            assert bool((lo <= hi).all())
            assert bool(((thr64 >= lo) & (thr64 <= hi)).all()), (k, p, int(((thr64 < lo) | (thr64 > hi)).sum()))
            assert bool((lg64 == thr64[..., None]).any(-1).all())
            if k:
                assert bool((thr64 >= dec.keep_threshold(lg64, T32, k, 1.0)).all())
            size = (lg64 >= thr64[..., None]).sum(-1)
            print(f"nucleus V={V} T={T} k={k} p={p}: kept {int(size.min())}..{int(size.max())}, "
                  f"bracket open in {int((lo != hi).sum())}/{lo.numel()} rows, d={d:.2e}")


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f"k{f[0]}p{f[1]}")
@pytest.mark.parametrize("T", [0.7, 1.0])
@pytest.mark.parametrize("V", [256, 1000])
def test_sampling_is_the_host_rule_on_the_device_threshold(V, T, filt):
    """token = first_argmax(where(lg >= threshold, lg / T + gumbel_noise, -inf))
    on the host in fp32, from the kernels' own logits and threshold.  As in
    test_gpu_decode.py, a draw whose two best host values lie within 1e-4 is
    left out, and at most 1 % may be."""
    H, E, L, B, N = 128, 64, 2, 16, 32
    model = _model(H, E, V, L, torch.bfloat16, seed=4, spread=2.0)
    first = torch.arange(B, device=_dev()) % V
    seed = 5
    tok, lg, _, _, thr, _ = _low(model, first, N, temperature=T, seed=seed, pos0=1, top_k=filt[0], top_p=filt[1])
    tok, lg, thr = tok.cpu(), lg.cpu(), thr.cpu()
    assert bool((thr > -INF).all())
    streams = torch.arange(B)
    out = 0
    for p in range(N):
        y = lg[:, p] / torch.tensor(T, dtype=torch.float32) + dec.gumbel_noise(seed, streams, 1 + p, V)
        y = torch.where(lg[:, p] >= thr[:, p, None], y, torch.full_like(y, -INF))
        top = y.topk(2, dim=-1).values
        sure = ~((top[:, 0] - top[:, 1]) < 1e-4)
        out += int((~sure).sum())
        assert torch.equal(tok[sure, p], dec.first_argmax(y)[sure]), p
    assert out <= (B * N) // 100, out


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
def test_every_workgroup_draws_the_same_token(cdt):
    """Free-running, all H / 4 workgroups draw the token and read their own
    embedding columns by it; forced to the recorded tokens, workgroup 0 alone
    draws.  Equal bits in tokens, logits, thresholds, log-probs, h and c: no
    workgroup fed another row."""
    H, E, V, L, B, N = 128, 64, 256, 2, 5, 12
    model = _model(H, E, V, L, cdt, seed=5, spread=2.0)
    first = torch.tensor([3, 1, 4, 1, 5], device=_dev())
    for k, p in FILTERS:
        kw = dict(temperature=0.9, seed=3, pos0=1, top_k=k, top_p=p)
        a = [x.clone() for x in _low(model, first, N, **kw)]
        b = [x.clone() for x in _low(model, first, N, **kw)]
        forced = torch.cat([first[:, None], a[0][:, :-1]], 1)
        f = _low(model, first, N, forced=forced, **kw)
        for x, y, z in zip(a, b, f):
            assert torch.equal(x, y) and torch.equal(x, z), (k, p)
        assert not torch.equal(a[0], _low(model, first, N, temperature=0.9, seed=3, pos0=1)[0])


def test_filters_off_is_the_plain_path():
    H, E, V, L, B, N = 128, 64, 256, 2, 5, 6
    model = _model(H, E, V, L, torch.bfloat16)
    prompt = torch.arange(B * 2).view(B, 2).to(_dev()) % V
    tok, lg = model.generate(prompt, N, temperature=0.8, seed=2, return_logits=True)
    for k in (0, V, V + 5):
        t, l = model.generate(prompt, N, temperature=0.8, seed=2, return_logits=True, top_k=k, top_p=1.0)
        assert torch.equal(t, tok) and torch.equal(l, lg), k
    # the filtered sampler with nothing to filter (asked for its outputs only) draws the same tokens
    t, l, lp = model.generate(prompt, N, temperature=0.8, seed=2, return_logits=True, return_logprobs=True)
    assert torch.equal(t, tok) and torch.equal(l, lg)
    # greedy ignores the filters
    g = model.generate(prompt, N, temperature=0.0)
    assert torch.equal(model.generate(prompt, N, temperature=0.0, top_k=3, top_p=0.5), g)


def test_batch_independence_with_filters():
    """A stream's tokens, thresholds and log-probs depend on its row index and
    on nothing else in the batch: B = 20 (groups of 16 and 4), 16, 1, and row
    17 alone through the op with its global index."""
    H, E, V, L, N = 128, 64, 256, 2, 5
    model = _model(H, E, V, L, torch.bfloat16, seed=5, spread=2.0)
    g = torch.Generator().manual_seed(2)
    first = torch.randint(0, V, (20,), generator=g).to(_dev())
    h0 = (0.5 * torch.randn(L, 20, H, generator=g)).to(_dev(), torch.bfloat16)
    c0 = torch.randn(L, 20, H, generator=g).to(_dev())
    kw = dict(temperature=1.0, seed=9, pos0=1, top_k=40, top_p=0.9)
    r20 = _groups(model, first, N, h0, c0, **kw)
    r16 = _groups(model, first[:16], N, h0[:, :16], c0[:, :16], **kw)
    r1 = _groups(model, first[:1], N, h0[:, :1], c0[:, :1], **kw)
    o = _low(model, first[17:18], N, h0[:, 17:18], c0[:, 17:18], stream0=17, **kw)
    for i, (x20, x16, x1) in enumerate(zip(r20, r16, r1)):
        assert torch.equal(x16, x20[:16]) and torch.equal(x1, x20[:1]), i
        assert torch.equal((o[0], o[4], o[5])[i], x20[17:18]), i
    assert not torch.equal(r20[0][16:17], r20[0][17:18])
    gt, glp = model.generate(first[:, None], N, temperature=1.0, seed=9, state=(h0, c0), top_k=40, top_p=0.9,
                             return_logprobs=True)
    assert torch.equal(gt, r20[0]) and torch.equal(glp, r20[2])


@pytest.mark.parametrize("top_k,top_p,kept", [(3, 1.0, [0, 1, 2]), (4, 1.0, [0, 1, 2, 3, 4]), (0, 0.6, [0, 1, 2])],
                         ids=["k3", "k4-keeps-5", "p0.6"])
def test_filtered_distribution_on_the_device(top_k, top_p, kept):
    """The 8-entry model of test_distribution_on_the_device, 16 x 256 draws,
    the seeds of test_decode_filter_cpu.py: nothing outside the kept set,
    chi-square below the 0.999 quantile at (kept - 1) degrees of freedom."""
    model = _model(64, 32, 8, 1, torch.bfloat16, seed=2)
    with torch.no_grad():
        for w in model.lstm.parameters():
            w.zero_()
        model.fc.weight.zero_()
        model.fc.bias.copy_(torch.tensor(P8).log())
    prompt = torch.zeros(16, 1, dtype=torch.int64, device=_dev())
    tok = model.generate(prompt, 256, temperature=1.0, seed=0, top_k=top_k, top_p=top_p).cpu()
    cnt = torch.bincount(tok.flatten(), minlength=8).double()
    p = torch.tensor(P8, dtype=F64)
    q = p[kept] / p[kept].sum()
    assert int(cnt.sum() - cnt[kept].sum()) == 0
    chi2 = float(((cnt[kept] - q * tok.numel()) ** 2 / (q * tok.numel())).sum())
    print(f"decode chi-square top_k={top_k} top_p={top_p}: {chi2:.2f}")
    assert chi2 < CHI2_999[len(kept) - 1]


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
def test_logprobs(cdt):
    """Against fp64 from the kernels' own logits and threshold, within
    (10 Y + 44) 2^-24 (module docstring); filters off: fp64 log_softmax(lg / T)
    at the token; greedy: the argmax's log-prob at T = 1, threshold -inf."""
    H, E, V, L, B, N = 64, 32, 1000, 1, 16, 8
    model = _model(H, E, V, L, cdt, seed=6, spread=1.5)
    first = torch.arange(B, device=_dev())
    worst = 0.0
    for T in (1.0, 0.7):
        T32 = float(torch.tensor(T, dtype=torch.float32))
        for k, p in [(0, 1.0)] + FILTERS:
            flats, bufs = _guarded_bufs(L, B, H, V, N, cdt)
            tok, lg, _, _, thr, lp = _low(model, first, N, bufs=bufs, temperature=T, seed=8, top_k=k, top_p=p)
            torch.cuda.synchronize()
            _assert_guards(flats)
            tok, lg64, thr64, lp64 = tok.cpu(), lg.double().cpu(), thr.double().cpu(), lp.double().cpu()
            Y = float(lg64.abs().max()) / T32
            assert Y <= 16
            bound = (10 * Y + 44) * U
            if (k, p) == (0, 1.0):
                assert bool((thr64 == -INF).all())
                want = torch.log_softmax(lg64 / T32, -1).gather(-1, tok[..., None])[..., 0]
            else:
                want = dec.token_logprobs(lg64, tok, T32, thr64)
            err = float((lp64 - want).abs().max())
            worst = max(worst, err / bound)
            assert err <= bound, (T, k, p, err, bound)
    print(f"decode log-prob worst |err| / bound {cdt}: {worst:.3f}")
    tok, lg, _, _, thr, lp = _low(model, first, N, temperature=0.0, top_k=3, top_p=0.5)
    assert torch.equal(tok, dec.first_argmax(lg)) and bool((thr == -INF).all())
    want = torch.log_softmax(lg.double(), -1).gather(-1, tok[..., None])[..., 0]
    assert float((lp.double() - want).abs().max()) <= (10 * float(lg.abs().max()) + 44) * U


def test_refusals_and_routing(monkeypatch):
    H, E, V, L, B, N = 64, 32, 24, 1, 3, 4
    model = _model(H, E, V, L, torch.float16)
    first = torch.tensor([1, 2, 3], device=_dev())
    f32 = dict(device=_dev(), dtype=torch.float32)
    for name in ("threshold", "logprobs"):
        for bad in (torch.empty(B, N + 1, **f32), torch.empty(B + 1, N, **f32), torch.empty(B * N, **f32),
                    torch.empty(B, N, device=_dev(), dtype=torch.float64), torch.empty(B, 2 * N, **f32)[:, ::2],
                    torch.empty(B, N)):
            bufs = dec.alloc_buffers(L, B, H, V, N, torch.float16, _dev(), True, True, True)
            bufs[name] = bad
            with pytest.raises(RuntimeError, match="threshold / logprobs"):
                _low(model, first, N, bufs=bufs)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            _low(model, first, N, **kw)
        with monkeypatch.context() as m:  # past the op's own check: the binding's
            m.setattr(dec, "check_filters", lambda *a: None)
            with pytest.raises(RuntimeError, match="top_k|top_p"):
                _low(model, first, N, **kw)
    torch.cuda.synchronize()

    # an fp32 model: no decode kernel -> the reference path, the same rule through the mirror
    torch.manual_seed(0)
    slow = CharLM(20, 16, 32, 2, compute_dtype=torch.float32).to(_dev())  # (a shape of this test's own: one warning per shape)
    with torch.no_grad():
        slow.fc.weight.mul_(8.0)
    prompt = torch.tensor([[2], [4], [6]], device=_dev())
    kw = dict(temperature=0.9, seed=1, top_k=5, top_p=0.8)
    with pytest.warns(RuntimeWarning, match="char-LM decode"):
        tok, lg, lp = slow.generate(prompt, 6, return_logits=True, return_logprobs=True, **kw)
    tau = dec.keep_threshold(lg, 0.9, 5, 0.8)
    assert bool((tau > -INF).all())
    for q in range(6):
        assert torch.equal(tok[:, q], dec.sample(lg[:, q], 0.9, 1, torch.arange(3), 1 + q, tau=tau[:, q]))
    want = dec.token_logprobs(lg.double(), tok, 0.9, tau.double())
    assert float((lp.double() - want).abs().max()) <= 1e-5
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    with pytest.raises(RuntimeError, match="strict"):
        slow.generate(prompt, 4, **kw)
    with pytest.raises(RuntimeError, match="strict"):  # a vocabulary the kernels do not cover
        CharLM(1040, 32, 64, 1, compute_dtype=torch.bfloat16).to(_dev()).generate(prompt, 2, **kw)


def test_stop_on_the_device():
    """``stop`` through generate on the fused path == the rule applied by hand
    to the tokens and log-probs of the same call without it."""
    H, E, V, L, B, N = 64, 32, 24, 1, 20, 24
    model = _model(H, E, V, L, torch.bfloat16, seed=8)
    prompt = torch.arange(B, device=_dev()).view(B, 1) % V
    kw = dict(temperature=1.0, seed=4, top_k=12, top_p=0.95, return_logprobs=True)
    tok, lp = model.generate(prompt, N, **kw)
    stop = int(tok[0, 2])
    stok, slg, slp, n = model.generate(prompt, N, stop=stop, return_logits=True, return_lengths=True, **kw)
    assert slg.shape == (B, N, V) and n.dtype == torch.int64 and n.device == tok.device
    tok, lp, stok, slp, n = tok.cpu(), lp.cpu(), stok.cpu(), slp.cpu(), n.cpu()
    assert int(n[0]) == min(int((tok[0] == stop).nonzero()[0]) + 1, 3)
    for b in range(B):
        hit = (tok[b] == stop).nonzero().flatten()
        length = int(hit[0]) + 1 if len(hit) else N
        assert int(n[b]) == length
        assert torch.equal(stok[b, :length], tok[b, :length]) and bool((stok[b, length:] == stop).all())
        assert torch.equal(slp[b, :length], lp[b, :length]) and bool((slp[b, length:] == 0).all())
    assert int(n.min()) < N
    with pytest.raises(ValueError):
        model.generate(prompt, N, stop=stop, forced=tok.to(_dev()))
    with pytest.raises(ValueError):
        model.generate(prompt, N, stop=V)
    assert _ext.require() is not None
