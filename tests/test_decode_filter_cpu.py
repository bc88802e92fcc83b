"""Top-k / nucleus filtering, log-probs and ``stop`` of char-LM generation on
the CPU: the rule's mirror (ops/decode.py:keep_threshold) against a plain
sort-and-walk implementation written here, the filtered sampler's
distribution, ``CharLM.generate``'s new outputs and the ``lm_cli generate``
flags.

``kept_ref`` below is the yardstick: one row at a time in Python floats, the
entries sorted by (value descending, index ascending), top-k by the k-th value,
the nucleus by walking runs of equal values.  It also plants each ``defect`` a
filter could have; ``test_planted_defects_are_rejected`` shows the comparison
used for the real mirror rejecting every one of them.
"""
import json
import math

import pytest
import torch

from pytorch_distributed_rnn_amd import lm_cli
from pytorch_distributed_rnn_amd.models.charlm import CharLM
from pytorch_distributed_rnn_amd.ops import decode as dec

F64 = torch.float64
INF = float("inf")
VS = [1, 8, 24, 64, 65, 256, 300, 512, 1000, 1024]
DEFECTS = ("index_tie_break", "p_before_k", "no_renormalisation", "strict_compare")
# 0.999 quantiles of chi-square
CHI2_999 = {2: 13.816, 4: 18.467}
P8 = [0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]


def kept_ref(row, T, k, p, defect=None):
    """The kept entries of one row (a list of floats) as a sorted index list."""
    assert defect is None or defect in DEFECTS
    V = len(row)
    order = sorted(range(V), key=lambda v: (-row[v], v))
    if T == 0:
        return sorted(order)
    top = max(row) / T
    w = [math.exp(x / T - top) for x in row]

    def top_k(keep):
        if not 0 < k < V or k > len(keep):
            return keep
        kth = row[keep[k - 1]]
        if defect == "index_tie_break":
            return keep[:k]
        if defect == "strict_compare":
            return [v for v in keep if row[v] > kth]
        return [v for v in keep if row[v] >= kth]

    def top_p(keep, base):
        if not p < 1:
            return keep
        target = p * math.fsum(w[v] for v in base)
        out, i = [], 0
        while i < len(keep):
            j = i + 1
            while defect != "index_tie_break" and j < len(keep) and row[keep[j]] == row[keep[i]]:
                j += 1
            out += keep[i:j]
            mass = math.fsum(w[v] for v in out)
            if (mass > target) if defect == "strict_compare" else (mass >= target):
                break
            i = j
        return out

    if defect == "p_before_k":
        first = top_p(order, order)
        return sorted(top_k(first))
    first = top_k(order)
    return sorted(top_p(first, order if defect == "no_renormalisation" else first))


def _rows(V, g):
    """fp64 rows [R, V]: continuous ones, ones drawn from a coarse grid (ties
    everywhere: at the k-th value and at the nucleus boundary for some (k, p)
    below), mixed signs throughout, -inf entries, and hand-planted ties."""
    cont = torch.randn(3, V, generator=g, dtype=F64) * 3
    grid = (torch.randn(3, V, generator=g, dtype=F64) * 2).round() / 2
    holes = torch.randn(2, V, generator=g, dtype=F64) * 3
    if V > 2:
        holes[:, torch.randperm(V, generator=g)[:V // 3]] = -INF
    plant = torch.randn(2, V, generator=g, dtype=F64)
    if V >= 8:  # the three largest distinct, then a run of four equal ones: k = 4, 5, 6 end inside the run
        plant[0, :3] = torch.tensor([5.0, 4.0, 3.0], dtype=F64)
        plant[0, 3:7] = 2.5
        plant[0, 7:] = plant[0, 7:].clamp(max=2.0)
        # two equal leaders holding most of the mass: the nucleus boundary falls between them
        plant[1] = plant[1].clamp(max=0.0)
        plant[1, V // 2] = plant[1, V - 1] = 6.0
    return torch.cat([cont, grid, holes, plant])


def _settings(V):
    ks = sorted({0, 1, 2, 4, 5, 6, min(40, V - 1), V - 1, V, V + 5} - {-1})
    return [(T, k, p) for T in (1.0, 0.7) for k in ks for p in (1.0, 0.95, 0.9, 0.5, 0.05)]


def _mismatches(V, defect=None):
    g = torch.Generator().manual_seed(1000 + V)
    rows = _rows(V, g)
    bad = 0
    for T, k, p in _settings(V):
        tau = dec.keep_threshold(rows, T, k, p)
        assert tau.dtype == F64 and tau.shape == (rows.shape[0],)
        kept = rows >= tau[:, None]
        for r in range(rows.shape[0]):
            want = kept_ref(rows[r].tolist(), T, k, p, defect)
            got = kept[r].nonzero().flatten().tolist()
            off = 0 < k < V or p < 1
            # the threshold is the smallest kept logit, -inf with both filters off
            tau_ok = float(tau[r]) == (min(rows[r, got].tolist()) if off else -INF)
            bad += got != want or (defect is None and not tau_ok)
    return bad


@pytest.mark.parametrize("V", VS)
def test_keep_threshold_against_sort_and_walk(V):
    assert _mismatches(V) == 0


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_are_rejected(defect):
    assert all(_mismatches(V, defect) > 0 for V in (24, 65, 256)), defect


def test_keep_threshold_edges():
    x = torch.tensor([[1.0, -2.0, 3.0, 3.0, -INF, 0.5]], dtype=F64)
    assert float(dec.keep_threshold(x, 1.0, 0, 1.0)) == -INF
    assert float(dec.keep_threshold(x, 0.0, 2, 0.5)) == -INF  # greedy ignores the filters
    assert float(dec.keep_threshold(x, 1.0, 1, 1.0)) == 3.0   # both leaders kept
    assert float(dec.keep_threshold(x, 1.0, 3, 1.0)) == 1.0
    assert float(dec.keep_threshold(x, 1.0, 5, 1.0)) == -2.0
    assert float(dec.keep_threshold(x, 1.0, 6, 1.0)) == -INF
    assert float(dec.keep_threshold(x, 1.0, 0, 0.5)) == 3.0   # 2 e^0 of 2 + e^-2 + e^-5 + e^-2.5: the pair is enough
    assert float(dec.keep_threshold(x, 1.0, 0, 0.95)) == 1.0
    assert dec.keep_threshold(x.float(), 1.0, 3, 0.9).dtype == torch.float32
    for k, p in ((-1, 1.0), (0, 0.0), (0, -0.5), (0, 1.5), (0, float("nan"))):
        with pytest.raises(ValueError):
            dec.keep_threshold(x, 1.0, k, p)


def test_top_k_one_is_greedy_and_wide_filters_are_none():
    g = torch.Generator().manual_seed(3)
    V, B = 65, 16
    logits = torch.randn(B, V, generator=g) * 3  # continuous: the top is untied
    streams = torch.arange(B)
    plain = dec.sample(logits, 0.8, 7, streams, 5)
    assert torch.equal(dec.sample(logits, 0.8, 7, streams, 5, top_k=1), dec.first_argmax(logits))
    assert not torch.equal(plain, dec.first_argmax(logits))
    for k in (V, V + 5, 0):
        assert torch.equal(dec.sample(logits, 0.8, 7, streams, 5, top_k=k, top_p=1.0), plain)
    # a kept token's noise does not depend on the filter: where the unfiltered draw is kept, it is the draw
    tau = dec.keep_threshold(logits, 0.8, 10, 0.9)
    filt = dec.sample(logits, 0.8, 7, streams, 5, top_k=10, top_p=0.9)
    inside = logits.gather(1, plain[:, None])[:, 0] >= tau
    assert bool(inside.any()) and torch.equal(filt[inside], plain[inside])
    assert bool((logits.gather(1, filt[:, None])[:, 0] >= tau).all())


def _p8_model():
    torch.manual_seed(2)
    model = CharLM(8, 32, 64, 1, compute_dtype=torch.float32)
    with torch.no_grad():
        for w in model.lstm.parameters():
            w.zero_()
        model.fc.weight.zero_()
        model.fc.bias.copy_(torch.tensor(P8).log())
    return model


@pytest.mark.parametrize("top_k,top_p,kept", [(3, 1.0, [0, 1, 2]), (4, 1.0, [0, 1, 2, 3, 4]), (0, 0.6, [0, 1, 2])],
                         ids=["k3", "k4-keeps-5", "p0.6"])
def test_filtered_sampling_fits_the_kept_distribution(top_k, top_p, kept):
    """16 x 256 = 4096 draws through ``generate`` from logits log p: no draw
    outside the kept set, chi-square against the renormalised kept
    probabilities below the 0.999 quantile at (kept - 1) degrees of freedom.
    top_k = 4 keeps five entries: the fourth largest is tied with the fifth.
    test_gpu_decode_filter.py draws the same seeds on the device."""
    tok, lp = _p8_model().generate(torch.zeros(16, 1, dtype=torch.int64), 256, temperature=1.0, seed=0, top_k=top_k,
                                   top_p=top_p, return_logprobs=True)
    cnt = torch.bincount(tok.flatten(), minlength=8).double()
    p = torch.tensor(P8, dtype=F64)
    q = p[kept] / p[kept].sum()
    assert int(cnt.sum() - cnt[kept].sum()) == 0
    chi2 = float(((cnt[kept] - q * tok.numel()) ** 2 / (q * tok.numel())).sum())
    print(f"chi-square top_k={top_k} top_p={top_p}: {chi2:.2f}")
    assert chi2 < CHI2_999[len(kept) - 1]
    want = torch.zeros(8, dtype=F64)
    want[kept] = q.log()
    torch.testing.assert_close(lp.double(), want[tok], rtol=0, atol=1e-6)


def test_logprobs_are_log_softmax_over_the_kept_set():
    g = torch.Generator().manual_seed(4)
    B, V = 12, 256
    logits = torch.randn(B, V, generator=g, dtype=F64) * 3
    tok = torch.randint(0, V, (B,), generator=g)
    for T, k, p in ((1.0, 0, 1.0), (0.7, 40, 1.0), (1.0, 0, 0.9), (0.7, 40, 0.9)):
        tau = dec.keep_threshold(logits, T, k, p)
        top = logits.topk(1).indices[:, 0]  # always kept
        want = torch.log_softmax(torch.where(logits >= tau[:, None], logits / T, torch.full_like(logits, -INF)), -1)
        for t in (top, torch.where(logits.gather(1, tok[:, None])[:, 0] >= tau, tok, top)):
            torch.testing.assert_close(dec.token_logprobs(logits, t, T, tau), want.gather(1, t[:, None])[:, 0],
                                       rtol=0, atol=1e-12)
    # greedy: the argmax's log-prob at T = 1, no filter
    got = dec.token_logprobs(logits, top, 0.0, dec.keep_threshold(logits, 0.0, 5, 0.5))
    torch.testing.assert_close(got, torch.log_softmax(logits, -1).gather(1, top[:, None])[:, 0], rtol=0, atol=1e-12)


def test_generate_outputs_follow_the_rule():
    """The reference path's tokens, thresholds and log-probs recomputed from
    its own logits."""
    torch.manual_seed(5)
    model = CharLM(40, 8, 12, 2, compute_dtype=torch.float32)
    with torch.no_grad():
        model.fc.weight.mul_(8.0)
    prompt = torch.tensor([[1, 2], [3, 4], [5, 6]])
    T, k, p, N = 0.9, 10, 0.8, 9
    tok, lg, lp, n, st = model.generate(prompt, N, temperature=T, seed=2, top_k=k, top_p=p, return_logits=True,
                                        return_logprobs=True, return_lengths=True, return_state=True)
    assert tok.shape == (3, N) and lg.shape == (3, N, 40) and lp.shape == (3, N) and lp.dtype == torch.float32
    assert n.tolist() == [N] * 3 and st[0].shape == (2, 3, 12)
    tau = dec.keep_threshold(lg, T, k, p)
    assert bool((tau > -INF).all()) and bool(((lg >= tau[..., None]).sum(-1) <= k).all())
    for q in range(N):
        assert torch.equal(tok[:, q], dec.sample(lg[:, q], T, 2, torch.arange(3), 2 + q, tau=tau[:, q]))
    torch.testing.assert_close(lp.double(), dec.token_logprobs(lg.double(), tok, T, tau.double()), rtol=0, atol=1e-5)
    # the op's own extra outputs
    out = dec.reference(model._step, None, prompt[:, -1], 4, temperature=T, seed=2, top_k=k, top_p=p,
                        return_threshold=True, return_logprobs=True, return_logits=True)
    model._state = None
    assert len(out) == 5 and torch.equal(out[3], dec.keep_threshold(out[1], T, k, p))
    # defaults: the call shapes and draws of before
    a = model.generate(prompt, N, temperature=T, seed=2)
    b = model.generate(prompt, N, temperature=T, seed=2, top_k=0, top_p=1.0)
    assert torch.equal(a, b) and not torch.equal(a, tok)


def test_stop_masks_tokens_and_logprobs():
    torch.manual_seed(6)
    model = CharLM(6, 8, 12, 1, compute_dtype=torch.float32)
    prompt = torch.zeros(8, 1, dtype=torch.int64)
    N = 24
    tok, lp = model.generate(prompt, N, seed=1, return_logprobs=True)
    stop = 3
    hits = tok == stop
    assert bool(hits.any(1).any()) and not bool(hits[:, 0].all())
    stok, slp, n, st = model.generate(prompt, N, seed=1, stop=stop, return_logprobs=True, return_lengths=True,
                                      return_state=True)
    for b in range(tok.shape[0]):
        first = hits[b].nonzero().flatten()
        length = int(first[0]) + 1 if len(first) else N
        assert int(n[b]) == length
        assert torch.equal(stok[b, :length], tok[b, :length]) and bool((stok[b, length:] == stop).all())
        assert torch.equal(slp[b, :length], lp[b, :length]) and bool((slp[b, length:] == 0).all())
    assert n.dtype == torch.int64 and st[0].shape == (1, 8, 12)
    # lengths without a stop token; a stop token that never comes
    assert model.generate(prompt, N, seed=1, return_lengths=True)[1].tolist() == [N] * 8
    g = model.generate(prompt, N, seed=1, top_k=1)
    absent = [v for v in range(6) if v not in g.flatten().tolist()]
    never = model.generate(prompt, N, seed=1, top_k=1, stop=absent[0], return_lengths=True)
    assert torch.equal(never[0], g) and never[1].tolist() == [N] * 8
    assert model.generate(prompt, 0, stop=stop, return_lengths=True)[1].tolist() == [0] * 8
    for bad in (dict(stop=stop, forced=tok), dict(stop=6), dict(stop=-1), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            model.generate(prompt, N, **bad)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A tiny model trained for two steps through the CLI."""
    d = tmp_path_factory.mktemp("charlm_filter")
    lm_cli.main(["--vocab", "128", "--embed", "16", "--hidden", "32", "--layers", "2", "--seq-len", "16",
                 "--batch-size", "4", "--synthetic-tokens", "4000", "--max-steps", "2", "--device", "cpu",
                 "--log", "WARNING", "--checkpoint-directory", str(d), "local"])
    return d / "charlm-epoch0.pt"


def _generate(checkpoint, tmp_path, *extra, name="out"):
    out, lpf = tmp_path / (name + ".bin"), tmp_path / (name + ".json")
    samples = lm_cli.main(["--checkpoint", str(checkpoint), "--device", "cpu", "--dtype", "fp32", "--log", "WARNING",
                           "--prompt", "ab", "--num-tokens", "48", "--samples", "6", "--seed", "3", "--output", str(out),
                           "--logprobs-file", str(lpf), *extra, "generate"])
    return samples, out.read_bytes(), json.loads(lpf.read_text())["samples"]


def test_generate_command_filters_and_stop(checkpoint, tmp_path, capsys):
    filt = ("--top-k", "5", "--top-p", "0.9")
    free, _, flp = _generate(checkpoint, tmp_path, *filt, name="free")
    assert all(len(s) == 48 for s in free) and all(len(e["logprobs"]) == 48 for e in flp)
    # byte 10, and a byte the samples are known to hold, so that samples do get cut
    for stop in (10, free[0][3]):
        capsys.readouterr()
        a, raw, lp = _generate(checkpoint, tmp_path, *filt, "--stop-token", str(stop), name=f"s{stop}")
        assert capsys.readouterr().out == "".join(s.decode("utf-8", errors="replace") + "\n" for s in a)
        assert raw == b"".join(a) and len(a) == len(lp) == 6
        for s, f, e, fe in zip(a, free, lp, flp):
            assert stop not in s and s == f.split(bytes([stop]))[0]  # the unstopped sample up to its first stop byte
            stopped = len(s) < 48
            assert e["length"] == len(s) + stopped and len(e["logprobs"]) == e["length"]
            assert e["logprobs"] == fe["logprobs"][:e["length"]]
            assert e["sum"] == pytest.approx(math.fsum(e["logprobs"]), abs=1e-9) and all(x <= 0 for x in e["logprobs"])
        b, _, lpb = _generate(checkpoint, tmp_path, *filt, "--stop-token", str(stop), name="again")
        assert a == b and lp == lpb
    assert len(a[0]) == 3  # sample 0 was cut before its fourth byte
    # the filters change the draw, and a token's probability among at most 5 beats its share of 128
    plain, _, plp = _generate(checkpoint, tmp_path, name="plain")
    assert plain != free
    assert sum(e["sum"] for e in flp) > sum(e["sum"] for e in plp)
    for bad in (("--top-k", "-1"), ("--top-p", "0"), ("--top-p", "1.5"), ("--stop-token", "128")):
        with pytest.raises(SystemExit):
            _generate(checkpoint, tmp_path, *bad, name="bad")
