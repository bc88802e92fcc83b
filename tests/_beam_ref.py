"""The beam-search rule of pdrnn/decode_rng.h as a sort-everything fp64
implementation, and the margin-form comparison the beam tests share.

``select`` lists every candidate of a group as Python floats and sorts the
list by (score descending, source beam, token): no torch sort, no tie handling
to get wrong.  ``check_selection`` judges ONE selection made in fp32 (by the
kernels, or by the fp32 mirror) against it, teacher-forced: from the scores,
the done flags and the logits that entered the selection.

The bound.  With u = 2^-24 (half an fp32 ulp), d_v = m - l_v >= 0, D the
largest finite d_v of the row and S = sum_v exp(-d_v) in [1, V], the kernel
computes lp_v = fl(fl(l_v - m) - logf(S~)) and cand = fl(cum + lp_v):

* fl(l_v - m) is off by u d_v <= u D;
* a weight expf(-d~_v) is off, relatively, by u d_v (its argument) + 2 u (expf,
  one ulp).  Weighted by p_v = w_v / S the argument terms sum to u E_p[d] and
  E_p[d] = H(p) - log S <= log V, so the exact sum of the computed weights is
  off by (log V + 2) u relative; adding them -- a lane's <= 16 in order, then
  the 6 levels of wave_sum, all terms >= 0 -- adds 21 u: S~ = S (1 + e),
  |e| <= (log V + 23) u;
* logf(S~): that e, plus one ulp of logf = 2 u log S <= 2 u log V;
* the difference's rounding: u |lp_v| <= u (D + log V);
* the sum's rounding: u |cand|.

Together |cand - cand64| <= eps = (2 D + 4 log V + 23 + C) u with C the
largest finite |cand64| of the selection (``eps`` below; 6.6e-6 at D = 30,
V = 256, C = 40).  Two fp32 scores whose fp64 values lie more than 2 eps apart
keep their order; closer ones may swap.
"""
import math

import torch

F64 = torch.float64
INF = float("inf")
U = 2.0 ** -24


def candidates(logits, cum, done, W, stop):
    """Every candidate of every group in fp64 -> a list per group of
    (score, j, v, lp), in (j, v) order; NaN scores as -inf."""
    l64 = logits.detach().to("cpu", F64)
    cum, done = cum.detach().to("cpu", F64).tolist(), [bool(x) for x in done.detach().cpu().tolist()]
    S, V = l64.shape
    lp = torch.log_softmax(l64, -1).tolist()
    out = []
    for g in range(S // W):
        cands = []
        for j in range(W):
            s = g * W + j
            if done[s]:
                if stop is not None:
                    cands.append((cum[s] if cum[s] == cum[s] else -INF, j, int(stop), 0.0))
                continue
            for v in range(V):
                c = cum[s] + lp[s][v]
                cands.append((c if c == c else -INF, j, v, lp[s][v]))
        out.append(cands)
    return out


def select(logits, cum, done, W, stop=None):
    """The rule by sorting everything -> (parent, token, cum, done, lp) like
    ops/decode.py:beam_select, fp64 on the CPU."""
    S = logits.shape[0]
    dn = [bool(x) for x in done.detach().cpu().tolist()]
    parent, token, ncum, ndone, nlp = [], [], [], [], []
    for g, cands in enumerate(candidates(logits, cum, done, W, stop)):
        best = sorted(cands, key=lambda c: (-c[0], c[1], c[2]))[:W]
        assert len(best) == W
        for c, j, v, lp in best:
            parent.append(g * W + j), token.append(v), ncum.append(c), nlp.append(lp)
            ndone.append(dn[g * W + j] or v == stop)
    return (torch.tensor(parent), torch.tensor(token), torch.tensor(ncum, dtype=F64), torch.tensor(ndone),
            torch.tensor(nlp, dtype=F64))


def eps(logits, cands):
    """The bound of the module docstring for one selection."""
    l64 = logits.detach().to("cpu", F64)
    d = l64.max(-1, keepdim=True).values - l64
    d = d[torch.isfinite(d)]
    D = float(d.max()) if d.numel() else 0.0
    C = max([abs(c[0]) for cs in cands for c in cs if math.isfinite(c[0])], default=0.0)
    return (2 * D + 4 * math.log(max(logits.shape[1], 2)) + 23 + C) * U


def check_selection(logits, cum, done, W, stop, parent, token, new_cum, new_done, new_lp=None, what=""):
    """Asserts the margin form for one selection (see the module docstring) and
    returns one dict per group: ``gap`` (the fp64 distance between the W-th and
    the (W + 1)-th best score; inf with no candidate left over, 0 between two
    -inf), ``eps`` and ``exact`` (gap > 2 eps: the selected set had to be, and
    was, the fp64 set)."""
    cands = candidates(logits, cum, done, W, stop)
    e = eps(logits, cands)
    parent, token = parent.detach().cpu().tolist(), token.detach().cpu().tolist()
    new_cum, new_done = new_cum.detach().cpu(), [bool(x) for x in new_done.detach().cpu().tolist()]
    dn = [bool(x) for x in done.detach().cpu().tolist()]
    bits = new_cum.contiguous().view(torch.int32 if new_cum.dtype == torch.float32 else torch.int64).tolist()
    nc = new_cum.to(F64).tolist()
    nlp = new_lp.detach().to("cpu", F64).tolist() if new_lp is not None else None
    out = []
    for g, cs in enumerate(cands):
        score = {(j, v): (c, lp) for c, j, v, lp in cs}
        sel = [(parent[g * W + i] - g * W, token[g * W + i]) for i in range(W)]
        assert len(set(sel)) == W, f"{what} group {g}: a candidate selected twice: {sel}"
        for i, k in enumerate(sel):
            assert k in score, f"{what} group {g} slot {i}: {k} is no candidate"
            want, lp = score[k]
            got = nc[g * W + i]
            got = -INF if got != got else got
            assert got == want or abs(got - want) <= e, f"{what} group {g} slot {i}: cum {got} != {want} (eps {e:.2e})"
            if nlp is not None and lp == lp:  # (a row of -inf logits has no log-probs)
                assert nlp[g * W + i] == lp or abs(nlp[g * W + i] - lp) <= e, f"{what} group {g} slot {i}: lp"
            assert new_done[g * W + i] == (dn[g * W + k[0]] or k[1] == stop), f"{what} group {g} slot {i}: done"
            if i:
                prev = nc[g * W + i - 1]
                assert prev >= got, f"{what} group {g}: scores rise at slot {i}"
                if bits[g * W + i - 1] == bits[g * W + i]:
                    assert sel[i - 1] < k, f"{what} group {g}: tie order at slot {i}: {sel[i - 1]} before {k}"
        ranked = sorted(cs, key=lambda c: (-c[0], c[1], c[2]))
        rest = [c[0] for c in cs if (c[1], c[2]) not in set(sel)]
        low = min(score[k][0] for k in sel)
        if rest:
            assert low >= max(rest) - 2 * e, f"{what} group {g}: selected {low} below an unselected {max(rest)} (eps {e:.2e})"
            a, b = ranked[W - 1][0], ranked[W][0]
            gap = 0.0 if a == b else a - b
        else:
            gap = INF
        exact = gap > 2 * e
        if exact:
            assert set(sel) == {(c[1], c[2]) for c in ranked[:W]}, f"{what} group {g}: not the fp64 set at gap {gap:.2e}"
        out.append({"gap": gap, "eps": e, "exact": exact})
    return out


def lm_model(H, E, V, L, cdt=torch.float32, seed=0, device="cpu", head_scale=8.0):
    """A CharLM whose head weights are scaled by 8: a default-initialised head
    is near uniform and its beam boundaries lie closer than fp32 resolves."""
    from pytorch_distributed_rnn_amd.models.charlm import CharLM
    torch.manual_seed(seed)
    model = CharLM(V, E, H, L, compute_dtype=cdt)
    with torch.no_grad():
        model.fc.weight.mul_(head_scale)
    return model.to(device)


# Full searches the CPU and GPU tests both run: (H, E, V, layers, G, W, N)
RUN_CASES = [(64, 32, 8, 2, 5, 3, 8), (64, 32, 8, 2, 1, 16, 8), (64, 32, 4, 1, 1, 16, 3), (64, 32, 65, 1, 3, 5, 8),
             (64, 32, 65, 1, 8, 2, 8), (128, 64, 256, 2, 1, 16, 8), (128, 64, 256, 2, 2, 8, 8), (128, 64, 256, 2, 16, 1, 6),
             (192, 96, 40, 3, 3, 5, 8), (192, 96, 40, 3, 4, 4, 7)]


def check_run(trace, W, stop, what=""):
    """check_selection at every position of a search's trace (tokens, parents,
    lp [S, N], cum, done [N + 1, S], logits [S, N, V]) -> the flat list of the
    per-(position, group) dicts."""
    out = []
    N = trace["tokens"].shape[1]
    for q in range(N):
        out += check_selection(trace["logits"][:, q], trace["cum"][q], trace["done"][q], W, stop, trace["parents"][:, q],
                               trace["tokens"][:, q], trace["cum"][q + 1], trace["done"][q + 1], trace["lp"][:, q],
                               what=f"{what} position {q}")
    return out


def ancestry(parents):
    """at [S, N]: the slot a final hypothesis occupied at each position's
    selection input, i.e. the slot whose logits selection q of it was made on."""
    S, N = parents.shape
    at = torch.empty(S, N, dtype=torch.int64)
    cur = torch.arange(S)
    par = parents.detach().cpu().to(torch.int64)
    for q in range(N - 1, -1, -1):
        cur = par[cur, q]
        at[:, q] = cur
    return at


def ancestry_logits(logits, parents):
    """[S, N, V]: for each final hypothesis the recorded logits it was
    selected from at every position."""
    at = ancestry(parents).to(logits.device)
    N = parents.shape[1]
    return torch.stack([logits[at[:, q], q] for q in range(N)], 1)


def planted_cases(V, G, W, seed=0):
    """The planted (logits [S, V] fp32, cum [S], done [S], stop) of the
    selection tests, by name: random rows; bit-identical rows with equal cum
    (exact ties across beams and inside a row); -inf scores and logits; done
    beams; every beam done; position 0's start scores."""
    S = G * W
    g = torch.Generator().manual_seed(1000 * V + 16 * G + W + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    stop = V // 2
    zeros = torch.zeros(S, dtype=torch.bool)
    cases = {}
    cases["random"] = (rnd(S, V) * 3, rnd(S) * 2 - 5, zeros, None)
    row = (rnd(1, V) * 2).round()  # integer logits: equal values inside the row too
    cases["ties"] = (row.expand(S, V).contiguous(), torch.full((S,), -3.0), zeros, None)
    lg = rnd(S, V) * 3
    lg[:, ::3] = -INF
    cum = rnd(S) - 4
    cum[1::2] = -INF
    cases["holes"] = (lg, cum, zeros, None)
    some = torch.arange(S) % 2 == 1
    cases["done"] = (rnd(S, V) * 3, rnd(S) - 4, some, stop)
    cases["done-ties"] = (row.expand(S, V).contiguous(), torch.full((S,), -3.0), some, stop)
    cases["all-done"] = (rnd(S, V) * 3, (rnd(S) - 4).sort(descending=True).values, ~zeros, stop)
    start = torch.full((G, W), -INF)
    start[:, 0] = 0
    cases["start"] = (rnd(S, V) * 3, start.reshape(S), zeros, stop)
    return cases
