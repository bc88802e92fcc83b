"""Fused inference path for the motion classifier on MI355X.

One batch of the model without gradients -- recurrent stack, classifier head,
argmax and, with labels, the cross-entropy statistics -- is ONE launch of the
sequence-in-wave forward's inference build (``lstm_head_infer``,
kernels/lstm_sw.hip): the training forward's step with nothing saved, the
head writing logits, predictions and one ``[loss / B, 1, correct]`` row per
sequence.  The rows are summed into a device accumulator by the deterministic
``col_sum`` kernels (no atomics), so an evaluation over many batches reads the
device once, at its end, instead of once per batch.

Serves what the sequence-in-wave family serves (H = 32, input size <= 12, one
or two unidirectional layers with biases, at most 16 classes); every other
model keeps ``model.forward``.  So does a batch whose sequences are too long
for any wave map's LDS (``lstm_sw_infer_plan`` refuses it: T above ~1360):
``MotionEvalStep`` runs that batch through ``model.forward`` and adds its
statistics into the same accumulator.
"""
from __future__ import annotations

import weakref
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .. import _ext
from ..ops.gemm import col_sum
from ..ops.gru_fused import PackBuffer


def _inner(model: nn.Module) -> nn.Module:
    return getattr(model, "module", model)


def supported(model: nn.Module, device: torch.device) -> bool:
    from ..models.motion import MotionModel
    m = _inner(model)
    device = torch.device(device)
    if device.type != "cuda" or not isinstance(m, MotionModel) or m.cell not in ("lstm", "gru"):
        return False
    mod = _ext.native(device)
    if mod is None or not hasattr(mod, "lstm_head_infer"):
        return False
    lstm = m.lstm
    # (lstm.dropout does not matter: evaluation applies none)
    if lstm.bidirectional or getattr(lstm, "proj_size", 0) or not lstm.bias:
        return False
    cell = 1 if m.cell == "gru" else 0
    if not mod.lstm_sw_ok(lstm.hidden_size, lstm.input_size, lstm.num_layers, cell):
        return False
    if m.fc.out_features > 16 or m.fc.in_features != lstm.hidden_size:
        return False
    params = list(m.parameters())
    if any(p.dtype != torch.float32 for p in params):
        return False
    if len({p.device for p in params}) != 1 or params[0].device.type != "cuda":
        return False  # (`device` may be a bare "cuda": the parameters say which GPU)
    cdt = getattr(m, "compute_dtype", torch.float32)
    if m.cell == "gru":
        return cdt == torch.float32  # the GRU runs the fp32 kernels only
    return cdt in (torch.float32, torch.bfloat16)


# model -> (what the verdict depends on, its MotionEvalStep or None), for
# step_for.  Weak keys; the step itself holds its model weakly.
_STEPS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def step_for(model: nn.Module) -> Optional["MotionEvalStep"]:
    """The model's cached ``MotionEvalStep`` (None: not served), so that a
    single ``predict`` call pays neither ``supported`` nor, for the GRU, a new
    packing buffer.  Asked again whenever the parameters' device or dtype or
    the model's compute dtype change (``.to()``, ``.double()``)."""
    m = _inner(model)
    w, r = m.fc.weight, getattr(m.lstm, "weight_hh_l0", None)
    key = (w.device, w.dtype, None if r is None else (r.device, r.dtype), getattr(m, "compute_dtype", None))
    ent = _STEPS.get(m)
    if ent is None or ent[0] != key:
        ent = (key, MotionEvalStep(m, checked=True) if supported(m, w.device) else None)
        _STEPS[m] = ent
    return ent[1]


class MotionEvalStep:
    """Callable running one inference batch: ``step(features, labels, idx)``
    returns ``(logits [B, C], pred [B])``; with labels the batch's
    ``[mean loss, n, correct]`` is added into a device accumulator, which
    ``result()`` reads (one device-to-host copy) and clears."""

    def __init__(self, model: nn.Module, checked: bool = False):
        """checked: the caller has just asked ``supported``."""
        m = _inner(model)
        dev = m.fc.weight.device
        if not checked and not supported(m, dev):
            raise RuntimeError("the fused motion inference path does not serve this model")
        self._m = weakref.ref(m)  # (whoever runs the step holds the model)
        self.mod = _ext.native(dev)
        self.H, self.NL = m.lstm.hidden_size, m.lstm.num_layers
        self.gru = m.cell == "gru"
        self.bf16 = getattr(m, "compute_dtype", torch.float32) == torch.bfloat16
        self.acc = None  # [sum of batch mean losses, examples, correct], made by the first labelled batch
        self.batches = 0
        self._gru_pack = PackBuffer()  # GRU: persistent [r|z|n_x|n_h] packing buffer

    @property
    def m(self) -> nn.Module:
        m = self._m()
        if m is None:
            raise RuntimeError("the model of this MotionEvalStep is gone")
        return m

    @property
    def weights(self):
        """The stack's parameters as they are now (read per call: a module's
        parameters may be replaced)."""
        lstm = self.m.lstm
        return [getattr(lstm, f"{k}_l{l}") for l in range(self.NL)
                for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]

    def _operands(self, features: Tensor):
        """(weights as the kernel reads them, features, cell code), as the
        fused train step: bf16 models round the fp32 masters in the kernel and
        read bf16 inputs; the GRU passes its packed 4-block stack, re-packed
        into a persistent buffer by one cat launch per batch (the fused
        optimizer writes the parameters through the flat buffer, so their
        version counters do not tell whether a packing is still current)."""
        ws = self.weights  # (no autograd here: the kernel takes the parameters as they are)
        if self.bf16:
            return ws, features if features.dtype == torch.bfloat16 else features.to(torch.bfloat16), 0
        if features.dtype != torch.float32:
            features = features.float()
        if not self.gru:
            return ws, features, 0
        return self._gru_pack.pack(ws, self.NL, self.H), features, 1

    @torch.no_grad()
    def __call__(self, features: Tensor, labels: Optional[Tensor] = None,
                 idx: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """features: the [N, T, I] table (gathered through idx inside the
        kernel) or the batch itself; labels: one per row of features."""
        if labels is not None:
            labels = labels.reshape(-1)
            if labels.dtype != torch.int64 or not labels.is_contiguous():
                labels = labels.long().contiguous()
        batch = idx.numel() if idx is not None else features.shape[0]
        try:
            self.mod.lstm_sw_infer_plan(self.NL, batch, features.shape[1])
        except RuntimeError:  # no wave map holds sequences this long in LDS
            return self._forward_batch(features, labels, idx)
        ws, features, cell = self._operands(features)
        if features.stride(2) != 1:
            features = features.contiguous()
        logits, pred, seq_stats, _, _ = self.mod.lstm_head_infer(
            features, idx, labels, ws, self.m.fc.weight, self.m.fc.bias, self.H, self.NL, cell, self.bf16, -1, False)
        if seq_stats is not None:
            if self.acc is None:
                self.acc = torch.zeros(3, dtype=torch.float32, device=seq_stats.device)
            col_sum(seq_stats, accumulate_into=[self.acc])
            self.batches += 1
        return logits, pred

    def _forward_batch(self, features: Tensor, labels: Optional[Tensor], idx: Optional[Tensor]):
        """A batch the kernels do not serve: ``model.forward`` in evaluation
        mode, argmax, and the cross-entropy kernel's [mean loss, n, correct]
        added into the accumulator on the device."""
        from ..ops.xent import cross_entropy_with_stats
        m = self.m
        was_training = m.training
        m.eval()
        try:
            logits = m(features, idx=idx)
        finally:
            m.train(was_training)
        if labels is not None:
            own = labels if idx is None else labels.index_select(0, idx)
            _, stats = cross_entropy_with_stats(logits, own)
            if self.acc is None:
                self.acc = torch.zeros(3, dtype=torch.float32, device=logits.device)
            self.acc.add_(stats.reshape(-1)[:3].to(torch.float32))
            self.batches += 1
        return logits, torch.argmax(logits, dim=1)

    def result(self) -> Tuple[float, int, int, int]:
        """(sum of the batches' mean losses, examples, correct, batches) since
        the last call: the one device-to-host read of an evaluation."""
        if self.acc is None:
            return 0.0, 0, 0, 0
        host = self.acc.cpu()
        out = (float(host[0]), int(round(float(host[1]))), int(round(float(host[2]))), self.batches)
        self.acc.zero_()
        self.batches = 0
        return out
