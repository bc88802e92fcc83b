#!/usr/bin/env python
"""SHA-256 of what the char-LM decode kernels compute.

    python tools/decode_digest.py [--full] [substring of the case names to run]

``ops.decode.decode`` and ``ops.decode.beam_decode`` on caller-made buffers,
on the models of tests/_beam_ref.py:lm_model, at the smallest shapes that
reach every kernel instantiation (plain, filtered and beam layer 0, the layers
above, both last launches; bf16 and fp16) and every rung of the slot ladder
(V = 8, 65, 200, 300, 1000); one JSON line per case with the digest of every
output buffer.  Two builds of the extension (PDRNN_EXT_SO selects one) compute
the same bits exactly when their outputs are equal line for line -- the check
for a refactor of the kernels.

``--full`` runs, for each of the ten models m (dtype x V; the stack (H, E, L)
is STACKS[m % 3]), every combination of B = 1 / 5 / 16, temperature 0 / 0.8,
the four filters, threshold and logprobs wanted or not, free-running or
forced (96 sampling cases), and of the four (G, W), stop on or off, log-probs
or not (16 search cases): 1120 lines.  Without it a model runs 4 sampling
cases, one per filter i = 0..3, with temperature TEMPERATURES[(i + m) % 2], B =
BATCHES[(i + m) % 3] and (wanted, forced) = EXTRAS[(i + m // 2) % 4], and 2
search cases i = 0, 1 with (G, W) = SEARCH[(2 i + m) % 4], stop on iff m // 4
is odd and log-probs iff m // 2 is odd: 60 lines, the set whose records are
kept (profiles/r16).  Over the ten models that holds every pair of sampling
settings and every (G, W) x stop x log-probs, but not every combination at
every model: a model sees one B, one temperature and one (wanted, forced) per
filter (so, e.g., at V = 300 in bf16 the one run with a filter on at T = 0.8
is forced and has B = 16), two of the four (G, W), and one stop / log-probs
setting.
"""
import hashlib
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from pytorch_distributed_rnn_amd import _ext  # noqa: E402
from pytorch_distributed_rnn_amd.ops import decode as dec  # noqa: E402
import _beam_ref as R  # noqa: E402

N = 8
VS = (8, 65, 200, 300, 1000)  # one per rung of the slot ladder
STACKS = ((64, 32, 1), (128, 64, 2), (64, 64, 3))  # (H, E, L), taken in turn over VS and the dtypes
FILTERS = ((0, 1.0), (3, 1.0), (0, 0.9), (3, 0.9))
# sampling, per model: every filter; the temperature, B, threshold / logprobs wanted and free-running / forced turn
# with the case and the model, so that the ten models together hold every pair of settings
TEMPERATURES = (0.0, 0.8)
BATCHES = (1, 5, 16)
EXTRAS = list(itertools.product((False, True), (False, True)))
# search, per model: two of the (G, W); with stop and return_logprobs the ten models hold every combination
SEARCH = ((1, 1), (2, 8), (5, 3), (1, 16))


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() if t is not None else None


def zeroed(bufs):
    for t in bufs.values():
        if t is not None:
            t.zero_()
    return bufs


def main():
    _ext.require()
    args = [a for a in sys.argv[1:] if a != "--full"]
    full, only = len(args) < len(sys.argv) - 1, args[0] if args else ""
    dev = torch.device("cuda", 0)
    for m, (cdt, V) in enumerate(itertools.product((torch.bfloat16, torch.float16), VS)):
        H, E, L = STACKS[m % len(STACKS)]
        model = R.lm_model(H, E, V, L, cdt, seed=H + V, device=dev)
        weights = (model.embedding.weight, model.lstm._weights(), model.fc.weight, model.fc.bias, cdt)
        g = torch.Generator().manual_seed(V + L)

        def state(B):
            return (0.5 * torch.randn(L, B, H, generator=g)).to(dev, cdt), torch.randn(L, B, H, generator=g).to(dev)

        tag = f"H{H} E{E} V{V} L{L} {str(cdt)[6:]}"
        sampling = [(T, B, e, i, f) for T in TEMPERATURES for B in BATCHES for e in EXTRAS for i, f in enumerate(FILTERS)]
        if not full:
            sampling = [(TEMPERATURES[(i + m) % 2], BATCHES[(i + m) % len(BATCHES)], EXTRAS[(i + m // 2) % len(EXTRAS)], i, f)
                        for i, f in enumerate(FILTERS)]
        for T, B, (wanted, force), i, (top_k, top_p) in sampling:
            name = f"sample {tag} B{B} T{T} k{top_k} p{top_p} outputs {int(wanted)} forced {int(force)}"
            h0, c0 = state(B)
            first = torch.randint(0, V, (B,), generator=g).to(dev)
            forced = torch.randint(0, V, (B, N), generator=g).to(dev) if force else None
            if only not in name:
                continue
            bufs = zeroed(dec.alloc_buffers(L, B, H, V, N, cdt, dev, True, wanted, wanted))
            out = dec.decode(*weights, h0, c0, first, N, temperature=T, seed=V + i, stream0=3, pos0=5, forced=forced,
                             return_logits=True, bufs=bufs, top_k=top_k, top_p=top_p, return_threshold=wanted,
                             return_logprobs=wanted)
            torch.cuda.synchronize()
            outs = dict(tokens=out[0], logits=out[1], threshold=bufs["threshold"], logprobs=bufs["logprobs"], h=out[2], c=out[3])
            print(json.dumps({"case": name, **{k: sha(v) for k, v in outs.items()}}), flush=True)
        search = list(itertools.product(SEARCH, (None, 3), (False, True)))
        if not full:
            search = [(SEARCH[(2 * i + m) % len(SEARCH)], (None, 3)[m // 4 % 2], bool(m // 2 % 2)) for i in range(2)]
        for (G, W), stop, lps in search:
            name = f"search {tag} G{G} W{W} stop {stop} logprobs {int(lps)}"
            h0, c0 = state(G)
            first = torch.randint(0, V, (G,), generator=g).to(dev)
            if only not in name:
                continue
            bufs = zeroed(dec.alloc_beam_buffers(L, G, W, H, V, N, cdt, dev, True, lps))
            dec.beam_decode(*weights, h0, c0, first, N, W, stop=stop, return_logits=True, return_logprobs=lps, bufs=bufs)
            torch.cuda.synchronize()
            keys = ("hyp", "hyp_lp", "cum", "done", "tokens", "parents", "lp", "logits")
            print(json.dumps({"case": name, **{k: sha(bufs[k]) for k in keys}, "h": sha(bufs["h"][N & 1]), "c": sha(bufs["c"])}),
                  flush=True)


if __name__ == "__main__":
    main()
