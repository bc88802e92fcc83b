#!/usr/bin/env python
"""SHA-256 of what every large-H recurrence kernel path computes.

    python tools/large_digest.py [substring of the case names to run]

One forward + backward through lstm_large_fwd / lstm_large_bwd per kernel
path and cell, at the shapes and input seeds of
tests/test_gpu_lstm_large_steps.py; one JSON line per case with the digest of
each of the six output tensors.  Two builds of the extension (PDRNN_EXT_SO
selects one) compute the same bits exactly when their outputs are equal line
for line -- the check for a refactor of the kernels.  The tune keys a case
needs are set per case; a build that reads `rows` once per process needs the
"fp32 bwd H 128" cases in a process of their own (the substring argument).
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from pytorch_distributed_rnn_amd import _ext  # noqa: E402
import test_gpu_lstm_large_steps as S  # noqa: E402

PP, PAIR, B16, ALL = {"large_pp": 2}, {"large_pp": 2, "large_pp_bwd": 2}, ("bf16", "fp16"), ("bf16", "fp16", "fp32")
# (name, H, B, T, ndir, mask, tile, storage types, tune keys)
CASES = [(f"fused step tile {t}", 128, 37, 3, 2, 2, t, ALL, {}) for t in range(5)]
CASES += [("fused step tile 3, two row blocks", 128, 300, 3, 2, 2, 3, ALL, {}),
          ("pp fwd / split-K 32x32 x2", 256, 300, 3, 2, 2, -1, B16, PP)]
CASES += [(f"split-K {form}", H, B, T, ndir, mask, tile, ALL, {}) for form, ((H, B, ndir, mask, T, tile), _) in S._SPLITK.items()]
CASES += [(f"pp GEMM + cell8 H {H}", H, 520, 3, ndir, mask, -1, B16, PAIR) for H, ndir, mask in ((512, 1, 0), (256, 2, 2))]
CASES += [(f"persistent 16-bit B {B}", 1024, B, 6, ndir, mask, -1, B16, {}) for B, ndir, mask in ((128, 1, 0), (200, 1, 0), (40, 2, 2))]
CASES += [(f"persistent fp32 bwd H {H} B {B}", H, B, T, ndir, mask, -1, ("fp32",), {} if H == 256 else {"rows": 0})
          for H in (256, 128) for B, T, ndir, mask in ((7, 4, 1, 1), (300, 3, 2, 2))]
CASES += [(f"row-owning fp32 B {B}", 128, B, 3, ndir, mask, -1, ("fp32",), {}) for B, ndir, mask in ((40, 2, 2), (200, 1, 0))]


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def main():
    mod = _ext.require()
    only = sys.argv[1] if len(sys.argv) > 1 else ""
    for name, H, B, T, ndir, mask, tile, dts, tune in CASES:
        if only not in name:
            continue
        os.environ["PDRNN_TUNE"] = ",".join(f"{k}={v}" for k, v in tune.items())
        for dt in dts:
            for cell in (0, 1):
                seed = H + 7 * B + 13 * T + 3 * cell + len("full")
                xp, w, wt, h0, c0, dout, dhn, dcn = S._inputs(H, B, T, ndir, dt, cell, "full", seed)
                hseq, cseq, acts = mod.lstm_large_fwd(xp, w, h0, c0, H, mask, tile, cell)
                dg, dh0, dc0 = mod.lstm_large_bwd(dout, dhn, dcn, wt, cseq, acts, c0, H, mask, tile, cell)
                torch.cuda.synchronize()
                outs = dict(hseq=hseq, cseq=cseq, acts=acts, dgates=dg, dh0=dh0, dc0=dc0 if cell == 0 else None)
                print(json.dumps({"case": name, "dt": dt, "cell": cell,
                                  **{k: sha(v) if v is not None else None for k, v in outs.items()}}), flush=True)
    mod.persist_check()


if __name__ == "__main__":
    main()
