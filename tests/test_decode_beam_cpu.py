"""Beam search on the CPU: ops/decode.py's mirror of the rule
(``beam_select``), the host-loop search (``beam_reference``),
``CharLM.beam_search`` on the reference path and ``lm_cli generate
--beam-width``.

The yardstick is tests/_beam_ref.py: the rule by sorting every candidate in
fp64, and the margin-form comparison (bound eps derived there) that
test_gpu_decode_beam.py applies to the kernels.  Here the comparison itself is
under test as well: it accepts the fp32 mirror on every case the GPU tests
use, and rejects five planted defects.
"""
import itertools
import json
import math

import pytest
import torch

from pytorch_distributed_rnn_amd import lm_cli
from pytorch_distributed_rnn_amd.ops import decode as dec

import _beam_ref as R

F64 = torch.float64
INF = float("inf")
SELECT_V = [1, 8, 63, 64, 65, 256, 300, 512, 1000, 1024]
SELECT_GW = [(1, 1), (16, 1), (1, 16), (5, 3), (2, 8), (3, 5)]


@pytest.mark.parametrize("V", SELECT_V)
def test_beam_select_against_sort_everything(V):
    """The fp64 mirror equals the sorted list exactly (parents, tokens, scores,
    done flags, log-probs); the fp32 mirror passes the margin form."""
    for (G, W) in SELECT_GW:
        for name, (lg, cum, done, stop) in R.planted_cases(V, G, W).items():
            want = R.select(lg, cum, done, W, stop)
            got = dec.beam_select(lg.to(F64), cum.to(F64), done, W, stop)
            for i, (x, y) in enumerate(zip(got, want)):
                assert torch.equal(x, y) or (i >= 2 and torch.allclose(x, y, rtol=0, atol=1e-12, equal_nan=True)), (name, G, W, i)
            got32 = dec.beam_select(lg, cum, done, W, stop)
            assert got32[2].dtype == torch.float32
            R.check_selection(lg, cum, done, W, stop, *got32, what=f"{name} V={V} G={G} W={W}")


def test_beam_select_edges():
    # V < W at the start: the real candidates, then -inf ones in (j, v) order
    lg = torch.tensor([[0.0, 1.0, -1.0]]).expand(4, 3).contiguous()
    parent, token, cum, done, lp = dec.beam_select(lg, dec.beam_start(1, 4), torch.zeros(4, dtype=torch.bool), 4, stop=1)
    assert parent.tolist() == [0, 0, 0, 1] and token.tolist() == [1, 0, 2, 0]
    assert cum[3] == -INF and done.tolist() == [True, False, False, False]
    assert torch.allclose(cum[:3], torch.log_softmax(lg[0], -1)[[1, 0, 2]])
    # a done beam keeps its score, emits stop with log-prob 0 and is not expanded
    parent, token, cum2, done2, lp = dec.beam_select(lg, cum, done, 4, stop=1)
    assert (parent[0], token[0], cum2[0], lp[0], done2[0]) == (0, 1, cum[0], 0.0, True)
    assert sorted(zip(parent.tolist(), token.tolist())).count((0, 1)) == 1 and (parent == 0).sum() == 1
    # NaN logits: the row's scores rank as -inf
    bad = lg.clone()
    bad[1, 0] = float("nan")
    parent, token, c3, _, _ = dec.beam_select(bad, torch.zeros(4), torch.zeros(4, dtype=torch.bool), 4)
    assert 1 not in parent.tolist() and not torch.isnan(c3).any()
    with pytest.raises(ValueError):
        dec.beam_select(lg, torch.zeros(4), torch.zeros(4, dtype=torch.bool), 3)
    for bad_kw in (dict(width=0), dict(width=17), dict(width=4, groups=5), dict(width=2, stop=3), dict(width=2, stop=-1),
                   dict(width=2, num_tokens=0)):
        with pytest.raises(ValueError):
            dec.check_beam(**{"stop": None, "V": 3, **bad_kw})


@torch.no_grad()
def _search(model, first, N, W, stop=None, select=dec.beam_select, gather=None, start=None, state=None):
    """beam_reference with replaceable parts: where the defects are planted."""
    G = first.shape[0]
    S = G * W
    src = torch.arange(G).repeat_interleave(W)
    tok = first[src]
    cum = dec.beam_start(G, W) if start is None else start
    done = torch.zeros(S, dtype=torch.bool)
    rec = {k: [] for k in ("tokens", "parents", "lp", "logits")}
    cums, dones = [cum], [done]
    state = tuple(x.index_select(1, src) for x in state) if state is not None else None
    kept = model._state
    for p in range(N):
        logits, state = model._step(tok.reshape(S, 1), state)
        logits = logits.float()
        parent, tok, cum, done, lp = select(logits, cum, done, W, stop)
        for k, x in zip(("tokens", "parents", "lp", "logits"), (tok, parent, lp, logits)):
            rec[k].append(x)
        cums.append(cum), dones.append(done)
        state = tuple(x.index_select(1, parent if gather is None else gather(parent)) for x in state)
    model._state = kept
    trace = {k: torch.stack(v, 1) for k, v in rec.items()}
    trace["cum"], trace["done"] = torch.stack(cums), torch.stack(dones)
    return trace


def _forced_logits(model, first, hyp, state=None):
    """The plain path's logits [S, N, V] when hypothesis s is fed to row s."""
    S, N = hyp.shape
    rep = first.repeat_interleave(S // first.shape[0])
    forced = torch.cat([rep[:, None], hyp[:, :-1]], 1)
    if state is not None:
        state = tuple(x.repeat_interleave(S // first.shape[0], dim=1) for x in state)
    return model.generate(rep[:, None], N, temperature=0.0, forced=forced, return_logits=True, state=state)[1]


@pytest.mark.parametrize("case", R.RUN_CASES, ids=lambda c: "H{}E{}V{}L{}G{}W{}N{}".format(*c))
def test_fp32_mirror_meets_the_bound_on_the_gpu_cases(case):
    """Every position of every search the GPU tests run, on the CPU in fp32:
    the margin form holds against fp64."""
    H, E, V, L, G, W, N = case
    model = R.lm_model(H, E, V, L, seed=H + V)
    first = torch.arange(G) % V
    trace = _search(model, first, N, W)
    res = R.check_run(trace, W, None, what=str(case))
    assert len(res) == N * G
    # beam_reference is this loop
    hyp, scores, hyp_lp, _, tr = dec.beam_reference(model._step, None, first, N, W, return_logprobs=True, return_trace=True)
    for k in trace:
        assert torch.equal(trace[k], tr[k]), k
    want, want_lp = dec.beam_backtrace(tr["tokens"], tr["parents"], tr["lp"])
    assert torch.equal(hyp.view(G * W, N), want) and torch.equal(hyp_lp.view(G * W, N), want_lp)
    assert torch.equal(scores.view(-1), tr["cum"][N])
    # the state gather: the logits along a hypothesis's ancestry are the plain path's on that hypothesis
    got = R.ancestry_logits(tr["logits"], tr["parents"])
    live = torch.isfinite(tr["cum"][N])
    assert float((got - _forced_logits(model, first, want))[live].abs().max()) < 1e-4


def test_boundary_gaps_resolve_in_fp32():
    """The condition that keeps the margin form from being vacuous: over all
    GPU cases, at least 90 % of the (case, position, group) triples have an
    fp64 gap at the beam boundary above 2 eps, where the selected set must be
    the fp64 set exactly."""
    res = []
    for (H, E, V, L, G, W, N) in R.RUN_CASES:
        model = R.lm_model(H, E, V, L, seed=H + V)
        res += R.check_run(_search(model, torch.arange(G) % V, N, W), W, None)
    exact = sum(r["exact"] for r in res)
    finite = [r["gap"] for r in res if 0 < r["gap"] < INF]
    print(f"beam boundary: {exact}/{len(res)} triples exact, smallest gap {min(finite):.2e}, "
          f"largest eps {max(r['eps'] for r in res):.2e}")
    assert exact >= 0.9 * len(res)


def _defect(name):
    def reversed_ties(lg, cum, done, W, stop):
        parent, token, c, d, lp = dec.beam_select(lg, cum, done, W, stop)
        out = [parent.clone(), token.clone(), c, d.clone(), lp.clone()]
        for i in range(len(c) - 1):
            if i // W == (i + 1) // W and c[i] == c[i + 1] and c[i] > -INF:
                for x in out[:2] + out[3:]:
                    x[[i, i + 1]] = x[[i + 1, i]]
                break
        else:
            raise AssertionError("no tie to reverse")
        return tuple(out)

    def done_expanded(lg, cum, done, W, stop):
        return dec.beam_select(lg, cum, torch.zeros_like(done), W, stop)

    def cum_dropped(lg, cum, done, W, stop):
        parent, token, c, d, lp = dec.beam_select(lg, cum, done, W, stop)
        return parent, token, lp.clone(), d, lp

    return {"tie order reversed": reversed_ties, "done beam expanded": done_expanded, "cum not carried": cum_dropped}[name]


@pytest.mark.parametrize("name", ["tie order reversed", "done beam expanded", "cum not carried"])
def test_the_comparison_rejects_a_wrong_selection(name):
    V, G, W = 8, 2, 4
    cases = R.planted_cases(V, G, W)
    lg, cum, done, stop = cases["ties" if name == "tie order reversed" else "done"]
    R.check_selection(lg, cum, done, W, stop, *dec.beam_select(lg, cum, done, W, stop))
    with pytest.raises(AssertionError):
        R.check_selection(lg, cum, done, W, stop, *_defect(name)(lg, cum, done, W, stop))


def test_the_comparison_rejects_a_wrong_gather_and_a_wrong_start():
    H, E, V, L, G, W, N = 64, 32, 8, 2, 2, 4, 6
    model = R.lm_model(H, E, V, L, seed=1)
    first = torch.tensor([1, 2])

    def mismatch(trace):
        hyp, _ = dec.beam_backtrace(trace["tokens"], trace["parents"])
        return float((R.ancestry_logits(trace["logits"], trace["parents"]) - _forced_logits(model, first, hyp)).abs().max())

    good = _search(model, first, N, W)
    assert any(p != list(range(g * W, g * W + W)) for q in range(1, N) for g in range(G)
               for p in [good["parents"][g * W:(g + 1) * W, q].tolist()])  # the parents do permute
    assert mismatch(good) < 1e-4
    assert mismatch(_search(model, first, N, W, gather=lambda parent: torch.arange(G * W))) > 1e-2
    # every copy of the prompt started at 0: position 0 selects the same token from several copies
    with pytest.raises(AssertionError):
        start = torch.zeros(G * W)
        bad = _search(model, first, N, W, start=start)
        bad["cum"][0] = dec.beam_start(G, W)  # (what the rule says entered position 0)
        R.check_run(bad, W, None)


def test_exhaustive_optimum():
    """V = 4, N = 3, W = 16: 16 prefixes prune nothing, so the search returns
    the 16 most likely of all 64 sequences, scored by fp64 teacher forcing."""
    V, N, W = 4, 3, 16
    model = R.lm_model(64, 32, V, 1, seed=3)
    first = torch.tensor([2])
    hyp, scores, _, _ = dec.beam_reference(model._step, None, first, N, W)
    seqs = torch.tensor(list(itertools.product(range(V), repeat=N)))
    lg = model.generate(first.expand(64, 1), N, temperature=0.0, return_logits=True,
                        forced=torch.cat([first.expand(64, 1), seqs[:, :-1]], 1))[1]
    total = torch.log_softmax(lg.to(F64), -1).gather(-1, seqs[..., None])[..., 0].sum(-1)
    best = total.sort(descending=True)
    assert float(best.values[W - 1] - best.values[W]) > 1e-4  # the boundary is resolved
    assert sorted(map(tuple, hyp[0].tolist())) == sorted(map(tuple, seqs[best.indices[:W]].tolist()))
    assert torch.allclose(scores[0].to(F64), best.values[:W], rtol=0, atol=1e-5)


def test_width_one_is_greedy():
    model = R.lm_model(64, 32, 65, 1, seed=4)
    prompt = torch.tensor([[3, 1, 4], [1, 5, 9], [2, 6, 5]])
    tok, lp = model.generate(prompt, 8, temperature=0.0, return_logprobs=True)
    hyp, scores, lengths, hlp = model.beam_search(prompt, 8, 1, return_logprobs=True)
    assert hyp.shape == (3, 1, 8) and hyp.dtype == torch.int64 and scores.dtype == torch.float32
    assert torch.equal(hyp[:, 0], tok) and bool((lengths == 8).all())
    assert torch.allclose(hlp[:, 0], lp, rtol=0, atol=1e-5) and torch.allclose(scores[:, 0], lp.sum(-1), rtol=0, atol=1e-4)


def test_stop_lengths_and_length_penalty():
    V, W, N = 8, 4, 8
    model = R.lm_model(64, 32, V, 2, seed=5)
    stop = 3
    with torch.no_grad():
        model.fc.bias[stop] += 0.5  # stop is likely: beams finish at different positions (lengths 1, 2 and 8)
    prompt = torch.tensor([[1, 2], [4, 5], [6, 7]])
    kept, mode = model._state, model.training
    hyp, scores, lengths, lp, state = model.beam_search(prompt, N, W, stop=stop, return_logprobs=True, return_state=True)
    assert model._state is kept and model.training == mode
    assert hyp.shape == (3, W, N) and lengths.dtype == torch.int64 and state[0].shape == (2, 3 * W, 64)
    assert int(lengths.min()) < N
    for b in range(3):
        for i in range(W):
            n = int(lengths[b, i])
            row = hyp[b, i].tolist()
            assert stop not in row[:n - 1] and (row[n - 1] == stop or n == N) and all(t == stop for t in row[n:])
            assert bool((lp[b, i, n:] == 0).all()) and bool((lp[b, i, :n] < 0).all())
            assert float(scores[b, i]) == pytest.approx(math.fsum(lp[b, i].tolist()), abs=1e-5)
        assert bool((scores[b, :-1] >= scores[b, 1:]).all())
    # the trace passes the margin form with done beams in it
    _, first_state = model._step(prompt[:, :-1], None)
    trace = _search(model, prompt[:, -1], N, W, stop=stop, state=first_state)
    assert bool(trace["done"].any()) and len(R.check_run(trace, W, stop)) == 3 * N
    # length penalty: a stable re-rank of the same hypotheses by score / length^a
    a = 1.5
    phyp, pscores, plengths = model.beam_search(prompt, N, W, stop=stop, length_penalty=a)
    for b in range(3):
        want = sorted(range(W), key=lambda i: (-(float(scores[b, i]) / float(lengths[b, i]) ** a), i))
        assert [hyp[b, i].tolist() for i in want] == phyp[b].tolist() and plengths[b].tolist() == lengths[b, want].tolist()
        assert torch.allclose(pscores[b], scores[b, want] / lengths[b, want].float() ** a)
    assert any(phyp[b].tolist() != hyp[b].tolist() for b in range(3))
    for bad in (dict(beam_width=0), dict(beam_width=17), dict(beam_width=2, stop=V), dict(beam_width=2, num_tokens=0)):
        with pytest.raises(ValueError):
            model.beam_search(prompt, **{"num_tokens": N, **bad})


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A tiny model trained for two steps through the CLI."""
    d = tmp_path_factory.mktemp("charlm_beam")
    lm_cli.main(["--vocab", "128", "--embed", "16", "--hidden", "32", "--layers", "2", "--seq-len", "16",
                 "--batch-size", "4", "--synthetic-tokens", "4000", "--max-steps", "2", "--device", "cpu",
                 "--log", "WARNING", "--checkpoint-directory", str(d), "local"])
    return d / "charlm-epoch0.pt"


def _generate(checkpoint, tmp_path, *extra, name="out"):
    out, lpf = tmp_path / (name + ".bin"), tmp_path / (name + ".json")
    samples = lm_cli.main(["--checkpoint", str(checkpoint), "--device", "cpu", "--dtype", "fp32", "--log", "WARNING",
                           "--prompt", "ab", "--num-tokens", "12", "--output", str(out), "--logprobs-file", str(lpf),
                           *extra, "generate"])
    return samples, out.read_bytes(), json.loads(lpf.read_text())["samples"]


def test_generate_command_beam_search(checkpoint, tmp_path, capsys):
    a, raw, lp = _generate(checkpoint, tmp_path, "--beam-width", "4", "--samples", "2")
    assert capsys.readouterr().out == "".join(s.decode("utf-8", errors="replace") + "\n" for s in a)
    assert len(a) == len(lp) == 2 and raw == b"".join(a) and all(len(s) == 12 for s in a)
    assert lp[0]["sum"] >= lp[1]["sum"]
    for e in lp:
        assert e["length"] == 12 and e["sum"] == pytest.approx(math.fsum(e["logprobs"]), abs=1e-4)
    b, _, lpb = _generate(checkpoint, tmp_path, "--beam-width", "4", "--samples", "2", "--seed", "9", name="again")
    assert a == b and lp == lpb  # a search: no seed in it
    # the best of 4 beams is at least as likely as greedy
    _, _, greedy = _generate(checkpoint, tmp_path, "--temperature", "0", name="greedy")
    assert lp[0]["sum"] >= greedy[0]["sum"] - 1e-4
    one, _, lp1 = _generate(checkpoint, tmp_path, "--beam-width", "1", name="one")
    assert lp1[0]["logprobs"] == pytest.approx(greedy[0]["logprobs"], abs=1e-5)
    s, _, slp = _generate(checkpoint, tmp_path, "--beam-width", "4", "--samples", "4", "--stop-token", str(a[0][2]),
                          "--length-penalty", "1.0", name="stop")
    assert all(a[0][2] not in x for x in s) and all(e["length"] == len(x) + (len(x) < 12) for x, e in zip(s, slp))
    for bad in (("--beam-width", "4", "--top-k", "5"), ("--beam-width", "4", "--top-p", "0.9"),
                ("--beam-width", "4", "--temperature", "0.5"), ("--beam-width", "17"), ("--beam-width", "2", "--samples", "3"),
                ("--length-penalty", "1.0"), ("--beam-width", "-1")):
        with pytest.raises(SystemExit):
            _generate(checkpoint, tmp_path, *bad, name="bad")
