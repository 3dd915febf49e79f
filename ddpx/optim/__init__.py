"""ddpx.optim."""
from __future__ import annotations

import torch

from .adamw import AdamW
from .ema import WeightEMA
from .lamb import LAMB
from .lars import LARS
from .sgd import SGD

__all__ = ["AdamW", "LAMB", "LARS", "SGD", "WeightEMA", "clip_grad_norm_", "decay_groups"]


def decay_groups(model, weight_decay: float):
    """The two parameter groups of the usual recipe "no weight decay on biases and BatchNorm": the parameters
    with ``ndim > 1`` (weight matrices, convolution filters) with ``weight_decay``, those with ``ndim <= 1`` with
    none.  Pass the result to any ``ddpx.optim`` optimizer built with ``allow_groups=True`` (or to torch's) in place of
    ``model.parameters()``.
    ``model``: a module, or an iterable of parameters."""
    params = list(model.parameters() if hasattr(model, "parameters") else model)
    return [{"params": [p for p in params if p.dim() > 1], "weight_decay": float(weight_decay)},
            {"params": [p for p in params if p.dim() <= 1], "weight_decay": 0.0}]


@torch.no_grad()
def clip_grad_norm_(model_or_params, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for a model in a flat parameter store (custom training loops).

    Computes the global L2 norm of the flat gradient (parameters only, never the alignment padding), scales
    the gradient buffer in place by ``min(1, max_norm / (norm + 1e-6))`` and returns the norm before clipping
    as a 0-d fp32 tensor on the store's device.  Nothing is read back to the host.  At world size > 1 call it
    after ``DistributedDataParallel.sync_grads()``: it clips the gradient this rank holds.

    ``ddpx.optim.sgd.SGD(max_grad_norm=...)`` does the same without rewriting the gradient (the factor is
    folded into the update); do not combine the two.
    """
    from ..ops.clip import GradNormPlan, scale_dev_
    from ..runtime.flat_params import flat_of
    flat = flat_of(model_or_params)
    if flat is None:
        raise ValueError("parameters are not flattened: wrap the model with ddpx.prepare_model() first")
    if not (flat.grad.is_cuda and torch.cuda.is_current_stream_capturing()):
        flat.fix_unwritten()  # a parameter nobody produced a gradient for counts as zero (torch: grad is None)
    plan = getattr(flat, "_clip_plan", None)
    if plan is None:
        plan = flat._clip_plan = GradNormPlan(flat)
    plan.compute(float(max_norm))
    scale_dev_(flat.grad, plan.coef_dev)
    return plan.norm_dev
