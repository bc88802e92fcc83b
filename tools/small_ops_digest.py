#!/usr/bin/env python
"""SHA-256 of what the small-H LSTM / GRU host layer computes.

    python tools/small_ops_digest.py TREE [substring of the case names to run]

TREE is the checkout to import the package from (this one: "."), so two
versions of the Python host code can run on ONE built extension
(PDRNN_EXT_SO): the check for a refactor of ops/lstm.py, ops/gru.py,
ops/gru_fused.py, train/fused_step.py and train/fused_eval.py.  One JSON line
per case with the digest of every output: for an operator case (through
models.rnn.LSTM / GRU, forward + backward) out, h_n, c_n, every parameter
gradient, dx and dh0 / dc0; for a MotionTrainStep case the statistics rows of
three consecutive steps and the flat parameter buffer after them; for a
MotionEvalStep case logits, predictions and result().  Strict kernel mode and
fixed seeds: two runs are equal line for line exactly when the bits are.
"""
import hashlib
import json
import os
import sys

import torch

os.environ["PDRNN_KERNELS"] = "hip-strict"
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from pytorch_distributed_rnn_amd.models.motion import MotionModel  # noqa: E402
from pytorch_distributed_rnn_amd.models.rnn import GRU, LSTM  # noqa: E402
from pytorch_distributed_rnn_amd.ops.adam import FusedAdam  # noqa: E402
from pytorch_distributed_rnn_amd.train.fused_eval import MotionEvalStep  # noqa: E402
from pytorch_distributed_rnn_amd.train.fused_step import MotionTrainStep  # noqa: E402
from pytorch_distributed_rnn_amd.utils.flat import flatten_module  # noqa: E402

DIRECT = dict(H=32, L=2)
# (name, cell, settings over I = 9, B = 6, T = 33, batch-first, bias, fp32, grad)
OPS = [("lstm direct", "lstm", DIRECT)]
OPS += [(f"lstm direct {k}", "lstm", dict(DIRECT, **{k: True}))
        for k in ("idx", "time_first", "state", "no_bias", "bf16", "nograd")]
OPS += [("lstm K-split B 1100", "lstm", dict(DIRECT, B=1100, T=8))]
OPS += [(f"lstm padded H {H}", "lstm", dict(H=H, L=2)) for H in (8, 24, 48)]
OPS += [("lstm L 5", "lstm", dict(H=32, L=5)), ("lstm L 3 dropout", "lstm", dict(H=32, L=3, dropout=0.5)),
        ("lstm bidir H 32 L 2", "lstm", dict(H=32, L=2, bidir=True)),
        ("lstm bidir H 16 L 1", "lstm", dict(H=16, L=1, bidir=True)),
        ("lstm H 100 padded large", "lstm", dict(H=100, L=1)),
        ("lstm H 128 idx", "lstm", dict(H=128, L=2, idx=True)),
        ("lstm H 128 idx time-first", "lstm", dict(H=128, L=2, idx=True, time_first=True)),
        ("gru H 32 L 2", "gru", DIRECT), ("gru H 8 L 2", "gru", dict(H=8, L=2)), ("gru H 48 L 3", "gru", dict(H=48, L=3)),
        ("gru dropout", "gru", dict(H=32, L=3, dropout=0.5)), ("gru state", "gru", dict(DIRECT, state=True)),
        ("gru no_bias", "gru", dict(DIRECT, no_bias=True)), ("gru nograd", "gru", dict(DIRECT, nograd=True))]


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def op_case(seed, cell, H, L, I=9, B=6, T=33, idx=False, time_first=False, state=False, no_bias=False, bf16=False,
            nograd=False, dropout=0.0, bidir=False):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    mod = (LSTM if cell == "lstm" else GRU)(I, H, L, bias=not no_bias, batch_first=not time_first, dropout=dropout,
                                            bidirectional=bidir).to(dev)
    mod.train(dropout > 0)
    N = B + 3 if idx else B
    x = torch.randn((T, N, I) if time_first else (N, T, I), device=dev)
    x = (x.bfloat16() if bf16 else x).requires_grad_(not nograd and not idx)  # (no input gradient through a gather)
    hx, states = None, []
    if state:
        states = [torch.randn(L, B, H, device=dev, requires_grad=True) for _ in range(2 if cell == "lstm" else 1)]
        hx = tuple(states) if cell == "lstm" else states[0]
    kw = {"idx": torch.randperm(N, device=dev)[:B]} if idx else {}
    if nograd:
        with torch.no_grad():
            out, st = mod(x, hx, **({"need_out": False} if cell == "lstm" else {}))
    else:
        out, st = mod(x, hx, **kw)
    hn, cn = st if cell == "lstm" else (st, None)
    res = {"out": sha(out), "h_n": sha(hn), "c_n": sha(cn)}
    if not nograd:
        loss = (out.float() * torch.randn_like(out, dtype=torch.float32)).sum() + hn.square().sum()
        if cn is not None:
            loss = loss + cn.sum()
        loss.backward()
        res.update({n: sha(p.grad) for n, p in mod.named_parameters()})
        res.update(dx=sha(x.grad), **{k: sha(s.grad) for k, s in zip(("dh0", "dc0"), states)})
    return res


def _motion(seed, cell, bf16):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    m = MotionModel(9, 32, 2, 6, cell=cell, compute_dtype=torch.bfloat16 if bf16 else torch.float32).to(dev)
    feats = torch.randn(256, 32, 9, device=dev)
    return m, feats, torch.randint(0, 6, (256,), device=dev)


def step_case(seed, cell, bf16, B):
    m, feats, labels = _motion(seed, cell, bf16)
    flatten_module(m)
    step = MotionTrainStep(m, FusedAdam(m.parameters(), lr=2.5e-3), None)
    res = {f"stats{k}": sha(step(feats, labels, torch.randperm(256, device=feats.device)[:B])) for k in range(3)}
    res["flat"] = sha(step.flat.data)
    return res


def eval_case(seed, cell):
    m, feats, labels = _motion(seed, cell, False)
    step = MotionEvalStep(m)
    logits, pred = step(feats, labels, torch.randperm(256, device=feats.device)[:37])
    return {"logits": sha(logits), "pred": sha(pred), "result": list(step.result())}


def main():
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    cases = [(name, op_case, (cell,), kw) for name, cell, kw in OPS]
    cases += [(f"train step {n} B {B}", step_case, (cell, bf16, B), {})
              for n, cell, bf16 in (("lstm", "lstm", False), ("gru", "gru", False), ("bf16", "lstm", True))
              for B in (37, 180)]
    cases += [(f"eval step {cell}", eval_case, (cell,), {}) for cell in ("lstm", "gru")]
    for seed, (name, fn, args, kw) in enumerate(cases):
        if only in name:
            res = fn(seed, *args, **kw)
            torch.cuda.synchronize()
            print(json.dumps({"case": name, **res}), flush=True)


if __name__ == "__main__":
    main()
