"""Evaluation: top-1 accuracy in percent, as the reference computes it.

``/root/reference/singlegpu.py:184-209``: ``@torch.inference_mode``,
``model.eval()``, iterate the test loader (tqdm "eval" bar), ``argmax(dim=1)``,
accumulate the correct count on the device, one ``.item()`` at the end.  Each
rank evaluates the full, unsharded test set on the unwrapped module
(``multigpu.py:247``).  Here the argmax/compare/count is one native kernel per
batch accumulating into a device int32 (a single D2H sync at the end).

:func:`evaluate_metrics` is the validation pass of a training run: loss, top-1 and top-k of the same loop, one
``ddpx.ops.head.eval_metrics`` launch per batch into device accumulators, one D2H read at the end (with
``tta_flip`` on the mean of the logits of each batch and of its mirror image).  Over a sharded
test loader (``DistributedIndexSampler(n, world, rank, shuffle=False)``) each rank evaluates its own samples, the
loader's ``valid_rows(step)`` keeps the sampler's padding out of the last batch, and one CPU float64 all-reduce on
``comm_group`` leaves every rank with the whole set's numbers.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import nn

from ..ops.elementwise import hflip
from ..ops.head import EvalAccumulator, accuracy_count, eval_metrics

try:
    from tqdm.auto import tqdm
except ImportError:  # pragma: no cover
    def tqdm(x, **_):
        return x


@torch.inference_mode()
def evaluate(model: nn.Module, dataflow, progress: bool = True) -> float:
    model.eval()
    num_samples = 0
    dev = None
    num_correct = None
    it = tqdm(dataflow, desc="eval", leave=False) if progress else dataflow
    for inputs, targets in it:
        if dev is None:
            dev = inputs.device
            num_correct = torch.zeros((), dtype=torch.int32, device=dev)
        outputs = model(inputs)
        accuracy_count(outputs, targets, num_correct)
        num_samples += targets.size(0)
    model.train()
    if num_samples == 0:
        return 0.0
    return (num_correct.double() / num_samples * 100).item()


class EvalResult(NamedTuple):
    loss: float             # mean cross-entropy over the samples
    top1: float             # percent
    topk: Optional[float]   # percent; None when no top-k was asked for
    k: int
    samples: int


@torch.inference_mode()
def evaluate_metrics(model: nn.Module, dataflow, topk: int = 0, comm_group=None, progress: bool = True,
                     tta_flip: bool = False) -> EvalResult:
    """Mean loss, top-1 and (``topk`` > 0) top-``topk`` accuracy of ``model`` over ``dataflow``.

    ``tta_flip`` (flip test-time augmentation): every batch is also forwarded as its mirror image
    (``ddpx.ops.elementwise.hflip`` in the loader's layout, ``dataflow.layout``; NCHW when the data flow names none)
    and the metrics launch scores the mean of the two logits (``eval_metrics(..., logits2=)``): two forwards, still
    one metrics launch per batch and one D2H read at the end.

    ``topk=0``: k = 1 and ``EvalResult.topk`` is None.  ``comm_group`` (a c10d group whose ranks each hold a shard
    of the test set): the sums are added over it, on the CPU, after the single device read.  The model is left in
    training mode, as :func:`evaluate` leaves it."""
    k = int(topk) if topk else 1
    model.eval()
    acc = None
    valid_rows = getattr(dataflow, "valid_rows", None)
    it = tqdm(dataflow, desc="eval", leave=False) if progress else dataflow
    for step, (inputs, targets) in enumerate(it):
        if acc is None:
            acc = EvalAccumulator(inputs.device)
        mv = int(valid_rows(step)) if valid_rows is not None else targets.size(0)
        if mv == 0:
            continue  # a batch of nothing but the sampler's padding
        if tta_flip:
            images = getattr(getattr(dataflow, "ds", None), "images", None)
            mirrored = hflip(inputs, getattr(dataflow, "layout", "nchw_f32"),
                             width=None if images is None else images.shape[-1])
            eval_metrics(model(inputs), targets, acc, k, mv, logits2=model(mirrored))
            continue
        eval_metrics(model(inputs), targets, acc, k, mv)
    model.train()
    loss_sum, hit1, hitk, rows = acc.read() if acc is not None else (0.0, 0, 0, 0)
    if comm_group is not None:
        import torch.distributed as dist
        t = torch.tensor([loss_sum, hit1, hitk, rows], dtype=torch.float64)
        dist.all_reduce(t, group=comm_group)  # CPU tensor: the c10d (gloo) group
        loss_sum, hit1, hitk, rows = float(t[0]), int(t[1]), int(t[2]), int(t[3])
    if rows == 0:
        return EvalResult(0.0, 0.0, 0.0 if topk else None, k, 0)
    return EvalResult(loss_sum / rows, hit1 / rows * 100, hitk / rows * 100 if topk else None, k, rows)
