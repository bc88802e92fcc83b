"""Beam search in the fused char-LM decode kernels (csrc/kernels/lstm_decode.hip:
beam_select, the BEAM instantiations of lstm_decode_layer, lstm_decode_beam_pick)
through ops/decode.py and CharLM.beam_search.

Selections are judged in the margin form of tests/_beam_ref.py, teacher-forced
per position: from the scores, done flags and logits the kernels themselves
recorded entering a position, every candidate is scored in fp64, and

* the lowest selected fp64 score >= the highest unselected one - 2 eps,
* each new score lies within eps of its candidate's fp64 score,
* the recorded order does not rise in the device's own scores, and is the
  rule's (source beam, then token, ascending) wherever two are bit-equal,
* where the fp64 gap at the beam boundary exceeds 2 eps the selected set is
  the fp64 set exactly -- and that must be so for >= 90 % of the (case,
  position, group) triples of the full runs, or the margin would hide
  everything.

eps is one position's error, derived from the kernel's arithmetic in
_beam_ref.py's docstring: (2 D + 4 log V + 23 + C) 2^-24 with D the largest
finite max - logit and C the largest finite |score| of the selection; the fp32
host mirror is shown to meet it on the same cases in test_decode_beam_cpu.py.
The models' head weights are scaled by 8 (``lm_model``): a default head is
near uniform and its boundaries lie closer than fp32 resolves.

The state gather is checked bit for bit: the logits recorded along a final
hypothesis's ancestry must equal those of the plain decode path forced to that
hypothesis from the same state -- any wrong h or c row, in any layer, at any
position, changes them.

Every buffer of a search sits between sentinel guard zones and starts
NaN-filled (floats) so that a value never written shows.

Measured on an MI355X when this file was written: 618 of the 622 (case,
position, group) triples of the full runs had to match fp64 exactly (the other
four are position 0 at V < W, whose boundary lies between two -inf), smallest
boundary gap 7.5e-5 against a largest eps of 5.3e-6; the W = 1 score differed
from the sum of greedy's log-probs by 4.3e-6 (bf16) / 3.3e-6 (fp16), bound
8.6e-5; every gather case found two swapped slots within its first two initial
states.  The 45 cases take 5 s.
"""
import functools
import itertools

import pytest
import torch

from pytorch_distributed_rnn_amd import _ext
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

import _beam_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
INF = float("inf")
U = 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 12288.0  # exact in bf16, fp16, fp32, int32 and int64
SELECT_V = [1, 8, 63, 64, 65, 256, 300, 512, 1000, 1024]
SELECT_GW = [(1, 1), (16, 1), (1, 16), (5, 3), (2, 8), (3, 5)]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _model(H, E, V, L, cdt, seed=0):
    return R.lm_model(H, E, V, L, cdt, seed=seed, device=_dev())


def _guarded(shape, dtype, rows=16):
    n = 1
    for s in shape:
        n *= s
    pad = rows * shape[-1]
    flat = torch.full((n + 2 * pad,), SENTINEL, device=_dev(), dtype=dtype)
    view = flat[pad:pad + n].view(shape)
    if dtype.is_floating_point:
        view.fill_(float("nan"))
    return flat, view, pad


def _guarded_bufs(L, G, W, H, V, N, cdt):
    S = G * W
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    shapes = {"h": ((2, L, S, H), cdt), "c": ((L, S, H), f32), "scratch": ((S, V), f32), "cum": ((N + 1, S), f32),
              "done": ((N + 1, S), i32), "tokens": ((S, N), i64), "parents": ((S, N), i32), "lp": ((S, N), f32),
              "logits": ((S, N, V), f32), "hyp": ((S, N), i64), "hyp_lp": ((S, N), f32)}
    flats, bufs = {}, {}
    for k, (shape, dt) in shapes.items():
        flat, view, pad = _guarded(shape, dt)
        flats[k], bufs[k] = (flat, pad), view
    return flats, bufs


def _assert_guards(flats):
    for k, (flat, pad) in flats.items():
        for zone in (flat[:pad], flat[-pad:]):
            assert bool((zone == SENTINEL).all()), f"{k}: a store outside the buffer"


def _run(model, first, N, W, stop=None, h0=None, c0=None, **kw):
    """A guarded search through the op -> (hyp, scores, hyp_lp, h, c), trace."""
    L, H, V = model.num_layers, model.hidden_dim, model.vocab_size
    flats, bufs = _guarded_bufs(L, first.shape[0], W, H, V, N, model.compute_dtype)
    out = dec.beam_decode(model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias,
                          model.compute_dtype, h0, c0, first, N, W, stop=stop, return_logits=True, return_logprobs=True,
                          bufs=bufs, **kw)
    torch.cuda.synchronize()
    _assert_guards(flats)
    trace = {k: bufs[k] for k in ("tokens", "parents", "lp", "cum", "done", "logits")}
    for k in ("lp", "cum", "logits", "hyp_lp", "c"):
        assert not bool(torch.isnan(bufs[k]).any()), f"{k}: a value never written"
    assert not bool(torch.isnan(bufs["h"][N & 1].float()).any())
    return out, trace


def _state(L, G, H, cdt, seed):
    g = torch.Generator().manual_seed(seed)
    return ((0.5 * torch.randn(L, G, H, generator=g)).to(_dev(), cdt), torch.randn(L, G, H, generator=g).to(_dev()))


@pytest.mark.parametrize("V", SELECT_V)
def test_select_kernel_on_planted_logits(V):
    """lstm_decode_beam_select -- the last position's kernel launched alone --
    on the planted cases of the CPU test, in the margin form; the exact-tie
    cases (integer logits, equal scores) must be the rule's list exactly."""
    mod = _ext.require()
    for (G, W) in SELECT_GW:
        S = G * W
        for name, (lg, cum, done, stop) in R.planted_cases(V, G, W).items():
            bufs = [_guarded(s, d) for s, d in (((S,), torch.int64), ((S,), torch.int32), ((S,), torch.float32),
                                                ((2, S), torch.float32), ((2, S), torch.int32))]
            got = mod.lstm_decode_beam_select(lg.to(_dev()), cum.to(_dev()), done.to(_dev()), W,
                                              -1 if stop is None else stop, out=[b[1] for b in bufs])
            torch.cuda.synchronize()
            for flat, _, pad in bufs:
                assert bool((flat[:pad] == SENTINEL).all()) and bool((flat[-pad:] == SENTINEL).all()), (name, G, W)
            parent, token, ncum, ndone, lp = got
            assert parent.dtype == torch.int64 and ndone.dtype == torch.bool and ncum.dtype == torch.float32
            R.check_selection(lg, cum, done, W, stop, parent, token, ncum, ndone, lp, what=f"{name} V={V} G={G} W={W}")
            if "ties" in name or name == "all-done":
                want = R.select(lg, cum, done, W, stop)
                assert torch.equal(parent.cpu(), want[0]) and torch.equal(token.cpu(), want[1]), (name, G, W)
                assert torch.equal(ndone.cpu(), want[3])
    # without out buffers, and the refusals
    lg = torch.randn(6, 40, device=_dev())
    a = mod.lstm_decode_beam_select(lg, torch.zeros(6, device=_dev()), torch.zeros(6, dtype=torch.bool, device=_dev()), 3)
    b = dec.beam_select(lg.double().cpu(), torch.zeros(6, dtype=F64), torch.zeros(6, dtype=torch.bool), 3)
    assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1])
    for bad in (dict(W=4), dict(W=0), dict(W=3, stop=40), dict(W=3, stop=-2)):
        with pytest.raises(RuntimeError):
            mod.lstm_decode_beam_select(lg, torch.zeros(6, device=_dev()), torch.zeros(6, dtype=torch.bool, device=_dev()),
                                        **bad)
    with pytest.raises(RuntimeError):
        mod.lstm_decode_beam_select(torch.randn(17, 8, device=_dev()), torch.zeros(17, device=_dev()),
                                    torch.zeros(17, dtype=torch.bool, device=_dev()), 1)
    with pytest.raises(RuntimeError):
        mod.lstm_decode_beam_select(torch.randn(2, 1025, device=_dev()), torch.zeros(2, device=_dev()),
                                    torch.zeros(2, dtype=torch.bool, device=_dev()), 1)


def _forced_plain(model, first, hyp, h0, c0, W):
    """The plain decode path's logits [S, N, V], row s forced to hypothesis s
    from its prompt's state."""
    S, N = hyp.shape
    rep = first.repeat_interleave(W)
    forced = torch.cat([rep[:, None], hyp[:, :-1]], 1)
    return dec.decode(model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias, model.compute_dtype,
                      h0.repeat_interleave(W, dim=1) if h0 is not None else None,
                      c0.repeat_interleave(W, dim=1) if c0 is not None else None, rep, N, temperature=0.0, forced=forced,
                      return_logits=True)[1]


def _has_swap(parents, W):
    """Two slots of a group that took each other's place at some selection."""
    par = parents.cpu().tolist()
    for q in range(len(par[0])):
        for i in range(len(par)):
            k = par[i][q]
            if k != i and par[k][q] == i:
                return True
    return False


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(64, 32, 65, 1, 3, 5, 8), (128, 64, 256, 2, 2, 8, 8), (192, 96, 40, 3, 1, 16, 8)],
                         ids=lambda c: "H{}E{}V{}L{}G{}W{}N{}".format(*c))
def test_state_gather_bit_for_bit(shape, cdt):
    """See the module docstring.  Several initial states are searched until
    the recorded parents hold a swap of two slots -- the case in which an
    in-place c update would read a row another lane has already replaced, were
    the load not complete before the store."""
    H, E, V, L, G, W, N = shape
    model = _model(H, E, V, L, cdt, seed=H)
    first = (torch.arange(G, device=_dev()) * 7 + 1) % V
    swapped = moved = False
    for seed in range(12):
        h0, c0 = _state(L, G, H, cdt, seed)
        (hyp, scores, hyp_lp, hn, cn), tr = _run(model, first, N, W, h0=h0, c0=c0)
        want = _forced_plain(model, first, hyp.view(G * W, N), h0, c0, W)
        got = R.ancestry_logits(tr["logits"], tr["parents"])
        assert torch.equal(got, want), seed
        # the hypotheses and their log-probs are the records traced back
        bt, bt_lp = dec.beam_backtrace(tr["tokens"], tr["parents"], tr["lp"])
        assert torch.equal(hyp.view(G * W, N), bt) and torch.equal(hyp_lp.view(G * W, N), bt_lp)
        assert torch.equal(scores.view(-1), tr["cum"][N])
        ident = torch.arange(G * W, device=_dev(), dtype=torch.int32)[:, None]
        moved = moved or bool((tr["parents"][:, 1:] != ident).any())
        swapped = swapped or _has_swap(tr["parents"], W)
        if swapped and seed >= 1:
            break
    print(f"beam gather {shape} {cdt}: parents moved {moved}, two slots swapped {swapped}, {seed + 1} states")
    assert moved and swapped


@functools.lru_cache(maxsize=None)
def _full_run(case, cdt):
    H, E, V, L, G, W, N = case
    model = _model(H, E, V, L, cdt, seed=H + V)
    out, tr = _run(model, torch.arange(G, device=_dev()) % V, N, W)
    return out, {k: v.cpu() for k, v in tr.items()}


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", R.RUN_CASES, ids=lambda c: "H{}E{}V{}L{}G{}W{}N{}".format(*c))
def test_every_selection_of_a_run(case, cdt):
    H, E, V, L, G, W, N = case
    _, tr = _full_run(case, cdt)
    res = R.check_run(tr, W, None, what=str(case))
    assert len(res) == N * G
    # the start: only beam 0 of a group is alive at position 0
    assert torch.equal(tr["cum"][0], dec.beam_start(G, W)) and not bool(tr["done"].any())
    assert bool((tr["parents"][:, 0].view(G, W)[:, :min(W, V)] == (torch.arange(G) * W)[:, None]).all())


def test_boundaries_are_resolved():
    """>= 90 % of the (case, position, group) triples of the full runs have an
    fp64 boundary gap above 2 eps and so were required to match fp64 exactly."""
    res = []
    for case in R.RUN_CASES:
        for cdt in DTYPES:
            res += R.check_run(_full_run(case, cdt)[1], case[5], None, what=str(case))
    exact = sum(r["exact"] for r in res)
    finite = [r["gap"] for r in res if 0 < r["gap"] < INF]
    print(f"beam boundary on the device: {exact}/{len(res)} triples exact, smallest gap {min(finite):.2e}, "
          f"largest eps {max(r['eps'] for r in res):.2e}")
    assert exact >= 0.9 * len(res)


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
def test_width_one_is_greedy(cdt):
    """Tokens bit for bit; the score is the sum of greedy's log-probs within N
    ((10 Y + 44) u [greedy's bound, test_gpu_decode_filter.py] + eps [the beam's
    log-prob] + u |score| [one addition])."""
    H, E, V, L, B, N = 128, 64, 256, 2, 16, 8
    model = _model(H, E, V, L, cdt, seed=2)
    prompt = torch.arange(B * 2, device=_dev()).view(B, 2) % V
    tok, lg, lp = model.generate(prompt, N, temperature=0.0, return_logits=True, return_logprobs=True)
    hyp, scores, lengths, hlp = model.beam_search(prompt, N, 1, return_logprobs=True)
    assert hyp.shape == (B, 1, N) and torch.equal(hyp[:, 0], tok) and bool((lengths == N).all())
    Y = float(lg.abs().max())
    bound = N * ((10 * Y + 44) * U + (4 * Y + 4 * 5.6 + 23 + float(scores.abs().max())) * U + U * float(scores.abs().max()))
    err = float((scores[:, 0].double() - lp.double().sum(-1)).abs().max())
    print(f"beam W=1 score vs greedy log-prob sum {cdt}: {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert float((hlp[:, 0].double() - lp.double()).abs().max()) <= bound / N


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
def test_exhaustive_optimum(cdt):
    """V = 4, N = 3, W = 16 prunes nothing: the result is the 16 best of all 64
    sequences, scored in fp64 from the plain path's forced logits, in the
    margin form with N positions' eps."""
    H, E, V, L, N, W = 64, 32, 4, 1, 3, 16
    model = _model(H, E, V, L, cdt, seed=3)
    first = torch.tensor([2], device=_dev())
    (hyp, scores, _, _, _), tr = _run(model, first, N, W)
    seqs = torch.tensor(list(itertools.product(range(V), repeat=N)), device=_dev())
    lg = torch.cat([_forced_plain(model, first.expand(16), seqs[i:i + 16], None, None, 1) for i in range(0, 64, 16)])
    total = torch.log_softmax(lg.double(), -1).gather(-1, seqs[..., None])[..., 0].sum(-1).cpu()
    Y = float(lg.abs().max())
    eps = N * (4 * Y + 4 * 1.39 + 23 + float(total.abs().max())) * U
    index = {tuple(s): i for i, s in enumerate(seqs.cpu().tolist())}
    sel = [index[tuple(h)] for h in hyp[0].cpu().tolist()]
    assert len(set(sel)) == W
    rest = [i for i in range(64) if i not in set(sel)]
    assert float(total[sel].min()) >= float(total[rest].max()) - 2 * eps
    assert float((scores[0].double().cpu() - total[sel]).abs().max()) <= eps
    best = total.sort(descending=True)
    if float(best.values[W - 1] - best.values[W]) > 2 * eps:
        assert set(sel) == set(best.indices[:W].tolist())
    assert bool((scores[0, :-1] >= scores[0, 1:]).all())


def test_groups_are_independent():
    """A group's hypotheses, scores and log-probs are the same bits alone, as
    group 0 and as group 4 of five; seven prompts (chunks of 5 + 2 at W = 3)
    equal the prompts run singly."""
    H, E, V, L, N, W = 128, 64, 256, 2, 6, 3
    model = _model(H, E, V, L, torch.bfloat16, seed=4)
    g = torch.Generator().manual_seed(1)
    first = torch.randint(0, V, (7,), generator=g).to(_dev())
    h0, c0 = _state(L, 7, H, torch.bfloat16, 5)
    five, _ = _run(model, first[:5], N, W, h0=h0[:, :5], c0=c0[:, :5])
    for at in (0, 4):
        alone, _ = _run(model, first[at:at + 1], N, W, h0=h0[:, at:at + 1], c0=c0[:, at:at + 1])
        for x, y in zip(alone[:3], five[:3]):
            assert torch.equal(x[0], y[at]), at
        for x, y in zip(alone[3:], five[3:]):
            assert torch.equal(x, y[:, at * W:(at + 1) * W]), at
    assert not torch.equal(five[0][0], five[0][4])
    out = model.beam_search(first[:, None], N, W, state=(h0, c0), return_logprobs=True, return_state=True)
    for b in range(7):
        one = model.beam_search(first[b:b + 1, None], N, W, state=(h0[:, b:b + 1], c0[:, b:b + 1]), return_logprobs=True,
                                return_state=True)
        for x, y in zip(one[:4], out[:4]):
            assert torch.equal(x[0], y[b]), b
        for x, y in zip(one[4], out[4]):
            assert torch.equal(x, y[:, b * W:(b + 1) * W]), b


@pytest.mark.parametrize("cdt", DTYPES, ids=["bf16", "fp16"])
def test_stop_lengths_and_length_penalty(cdt):
    H, E, V, L, N, W, B = 64, 32, 8, 2, 8, 4, 4
    model = R.lm_model(H, E, V, L, cdt, seed=5, device=_dev())
    stop = 3
    with torch.no_grad():
        model.fc.bias[stop] += 0.5  # stop is likely: beams finish at different positions
    first = torch.tensor([1, 4, 6, 7], device=_dev())
    (hyp, scores, hyp_lp, _, _), tr = _run(model, first, N, W, stop=stop)
    tr = {k: v.cpu() for k, v in tr.items()}
    assert len(R.check_run(tr, W, stop)) == B * N
    done, cum, par, tok, lp = tr["done"].bool(), tr["cum"], tr["parents"].long(), tr["tokens"], tr["lp"]
    assert bool(done[N].any()) and not bool(done[1].all())  # beams finish, and not all at once
    for q in range(N):  # a done beam's continuation: the same score, stop, log-prob 0
        was = done[q][par[:, q]]
        assert torch.equal(cum[q + 1][was], cum[q][par[:, q]][was])
        assert bool((tok[:, q][was] == stop).all()) and bool((lp[:, q][was] == 0).all())
        assert torch.equal(done[q + 1], was | (tok[:, q] == stop))
    out = model.beam_search(first[:, None], N, W, stop=stop, return_logprobs=True)
    assert torch.equal(out[0], hyp) and torch.equal(out[1], scores) and torch.equal(out[3], hyp_lp)
    hyp, scores, lengths, hlp = (x.cpu() for x in out)
    assert int(lengths.min()) < N and lengths.dtype == torch.int64
    for b in range(B):
        for i in range(W):
            n, row = int(lengths[b, i]), hyp[b, i].tolist()
            assert stop not in row[:n - 1] and (row[n - 1] == stop or n == N) and all(t == stop for t in row[n:])
            assert bool((hlp[b, i, n:] == 0).all())
            assert abs(float(scores[b, i]) - float(hlp[b, i].double().sum())) <= N * U * max(1.0, abs(float(scores[b, i])))
    a = 1.5
    phyp, pscores, plengths = (x.cpu() for x in model.beam_search(first[:, None], N, W, stop=stop, length_penalty=a))
    ranked = scores / lengths.float() ** a
    for b in range(B):
        want = sorted(range(W), key=lambda i: (-float(ranked[b, i]), i))
        assert [hyp[b, i].tolist() for i in want] == phyp[b].tolist() and plengths[b].tolist() == lengths[b, want].tolist()
        assert torch.allclose(pscores[b], ranked[b, want], rtol=1e-6, atol=0)
    assert any(phyp[b].tolist() != hyp[b].tolist() for b in range(B))


def test_repeatable():
    """The same bits again in every output and every trace buffer."""
    H, E, V, L, G, W, N = 128, 64, 256, 2, 2, 8, 8
    model = _model(H, E, V, L, torch.float16, seed=6)
    first = torch.tensor([5, 9], device=_dev())
    h0, c0 = _state(L, G, H, torch.float16, 2)
    runs = [_run(model, first, N, W, stop=7, h0=h0, c0=c0) for _ in range(2)]
    for out, tr in runs[1:]:
        for x, y in zip(out, runs[0][0]):
            assert torch.equal(x, y)
        for k in tr:
            assert torch.equal(tr[k], runs[0][1][k]), k


def test_refusals_and_routing(monkeypatch):
    mod = _ext.require()
    ok = (2, 8, 64, 32, 1024, 2, 0)
    assert mod.lstm_decode_beam_supported(*ok) and mod.lstm_decode_beam_supported(1, 16, 1024, 256, 256, 5, 1)
    for k, bad in ((0, 3), (0, 0), (1, 0), (1, 17), (1, -1), (2, 96), (3, 24), (4, 1025), (6, 2)):
        args = list(ok)
        args[k] = bad
        assert not mod.lstm_decode_beam_supported(*args), args
    model = _model(64, 32, 8, 2, torch.bfloat16)
    first = torch.tensor([1, 2], device=_dev())

    def low(first, N, W, **kw):
        return dec.beam_decode(model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias,
                               torch.bfloat16, None, None, first, N, W, **kw)

    bads = ((first, 4, 0, {}), (first, 4, 17, {}), (first, 4, 9, {}), (first, 4, 2, dict(stop=8)), (first, 4, 2, dict(stop=-1)),
            (first, 0, 2, {}))
    for f, N, W, kw in bads:
        with pytest.raises(ValueError):
            low(f, N, W, **kw)
        if W != 9:  # (the model runs 16 // 9 = 1 prompt per call)
            with pytest.raises(ValueError):
                model.beam_search(f[:, None], N, W, **kw)
    with monkeypatch.context() as m:  # past the op's own check: the binding's (where stop = -1 means none)
        m.setattr(dec, "check_beam", lambda *a, **k: None)
        for f, N, W, kw in (bads[2], bads[3], bads[5]):
            bufs = dec.alloc_beam_buffers(2, 2, W, 64, 8, max(N, 1), torch.bfloat16, _dev())
            if N == 0:
                bufs["tokens"] = bufs["tokens"][:, :0]
            with pytest.raises(RuntimeError, match="lstm_decode_beam"):
                low(f, N, W, bufs=bufs, **kw)
    torch.cuda.synchronize()

    calls = []
    real = dec.beam_decode
    monkeypatch.setattr(dec, "beam_decode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    prompt = torch.tensor([[2], [4], [6]], device=_dev())
    # fp32: no decode kernel -> the reference path (a warning), the mirror's results
    slow = R.lm_model(32, 16, 20, 2, torch.float32, seed=0, device=_dev())
    with pytest.warns(RuntimeWarning, match="char-LM beam search"):
        hyp, scores, lengths = slow.beam_search(prompt, 5, 4)
    assert not calls and hyp.shape == (3, 4, 5)
    ref = dec.beam_reference(slow._step, None, prompt[:, -1], 5, 4)
    assert torch.equal(hyp, ref[0]) and torch.equal(scores, ref[1])
    covered = model.beam_search(prompt[:, :1] % 8, 4, 4)
    assert calls == [1] and covered[0].shape == (3, 4, 4)
    monkeypatch.setenv("PDRNN_KERNELS", "hip-strict")
    with pytest.raises(RuntimeError, match="strict"):
        slow.beam_search(prompt, 4, 4)
    with pytest.raises(RuntimeError, match="strict"):  # a vocabulary the kernels do not cover
        CharLM(1025, 32, 64, 1, compute_dtype=torch.bfloat16).to(_dev()).beam_search(prompt, 2, 4)
    assert torch.equal(model.beam_search(prompt[:, :1] % 8, 4, 4)[0], covered[0])  # the kernels, in strict mode too


def test_beam_search_reads_updated_weights():
    """In-place updates of the masters (an optimizer step) reach the 16-bit
    copies the kernels read: the same bits as a fresh model with those weights."""
    H, E, V, L = 64, 32, 24, 2
    model = R.lm_model(H, E, V, L, torch.bfloat16, seed=3, device=_dev())
    prompt = torch.tensor([[1, 2], [3, 4]], device=_dev())
    before = model.beam_search(prompt, 4, 5, return_logprobs=True)
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(0.5).add_(0.01)
    after = model.beam_search(prompt, 4, 5, return_logprobs=True)
    fresh = CharLM(V, E, H, L, compute_dtype=torch.bfloat16).to(_dev())
    fresh.load_state_dict(model.state_dict())
    want = fresh.beam_search(prompt, 4, 5, return_logprobs=True)
    assert not torch.equal(after[3], before[3])
    for x, y in zip(after, want):
        assert torch.equal(x, y)
