"""Soft classification targets: label smoothing and the two-label mix of Mixup / CutMix.

Row m's target distribution over the C classes is

    q_c = (1 - eps) * (lam_m [c == a_m] + (1 - lam_m) [c == b_m]) + eps / C

with a = the batch's targets, b = ``tgt_b``, lam = ``lam`` and eps = ``label_smoothing``; the loss is
``lse_m - sum_c q_c z_c`` and its logit gradient ``(softmax - q) / M`` — ``F.cross_entropy(z, q_mix,
label_smoothing=eps)`` with probability targets.  The native heads form q inside their one launch
(``ddpx_head_fwd_soft`` / ``ddpx_f32_head_fwd_soft``); the functions here are the torch twin the CPU path and
the models without a native loss use.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


class SoftTargets:
    """Holder of the soft-target inputs of a loss: ``tgt_b`` (int64 [M] second labels, or None), ``lam``
    (fp32 [M] weight of the first label, or None for 1) and the ``label_smoothing`` scalar.  The tensors may be
    longer than the batch (persistent loader buffers): the first M elements are used."""

    __slots__ = ("tgt_b", "lam", "label_smoothing")

    def __init__(self, tgt_b=None, lam=None, label_smoothing: float = 0.0):
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError("label_smoothing must be in [0, 1]")
        if tgt_b is not None and tgt_b.dtype != torch.int64:
            raise ValueError("SoftTargets: tgt_b must be int64")
        if lam is not None and lam.dtype != torch.float32:
            raise ValueError("SoftTargets: lam must be fp32")
        self.tgt_b = tgt_b
        self.lam = lam
        self.label_smoothing = float(label_smoothing)

    def check(self, M: int, device):
        for name, t in (("tgt_b", self.tgt_b), ("lam", self.lam)):
            if t is not None and (t.device != device or t.numel() < M or not t.is_contiguous()):
                raise ValueError(f"SoftTargets: {name} must be a contiguous tensor of >= {M} elements on {device}")


def mixed_targets(targets, C: int, soft: SoftTargets, dtype=torch.float32):
    """[M, C] distribution lam [c == a] + (1 - lam) [c == b] (the smoothing is left to ``F.cross_entropy``)."""
    M = targets.numel()
    q = F.one_hot(targets, C).to(dtype)
    if soft.tgt_b is None:
        return q
    lam = soft.lam[:M].to(dtype)[:, None] if soft.lam is not None else torch.ones((M, 1), dtype=dtype,
                                                                                  device=targets.device)
    return lam * q + (1 - lam) * F.one_hot(soft.tgt_b[:M], C).to(dtype)


def soft_cross_entropy(logits, targets, soft: SoftTargets | None):
    """Batch-mean cross-entropy of ``logits`` against the soft targets (torch ops; differentiable)."""
    if soft is None:
        return F.cross_entropy(logits, targets)
    q = mixed_targets(targets, logits.shape[1], soft, logits.dtype)
    return F.cross_entropy(logits, q, label_smoothing=soft.label_smoothing)


def soft_dlogits(logits, targets, soft: SoftTargets):
    """(softmax - q) / M, the gradient of :func:`soft_cross_entropy`."""
    M, C = logits.shape
    eps = soft.label_smoothing
    q = (1.0 - eps) * mixed_targets(targets, C, soft, logits.dtype) + eps / C
    return (torch.softmax(logits, 1) - q) / M
