"""Exponential moving average (EMA) of the weights of a flat parameter store.

``WeightEMA(optimizer, decay=0.999, warmup=False, every=1)`` attaches to a :class:`ddpx.optim.flat.FlatOptimizer`
(SGD, AdamW, LARS or LAMB) and sets ``optimizer.ema``; the companion of ``torch.optim.swa_utils.AveragedModel`` /
timm's ``ModelEmaV2`` for a model in a flat store:

* the average is one more fp32 buffer laid out like the master, ``flat.state_tensors["ema"]`` (:attr:`buffer`): a
  sharded re-layout moves it with its parameters and ``DistributedDataParallel.consolidate()`` all-gathers it, as
  they do the optimizers' states.  It starts as a copy of the master (:meth:`reset`);
  ``DistributedDataParallel`` broadcasts it from rank 0 together with the weights, so every rank starts from rank
  0's;
* the update is ``ddpx_ema_flat`` (``csrc/kernels/ema.hip``), ``e += (p - e) * w``: one streaming launch at the end
  of the optimizer's step driver, on the stream the step's updates ran on and before that stream is joined back, so
  it stays inside a captured step.  Local and replicated-overlap schedules: one launch over the whole store, which
  covers parameters the fused backward kernels stepped and parameters without a gradient (as ``AveragedModel``
  does).  ZeRO-1: one launch per range this rank updates (``update_ranges(b)`` of every bucket); the rest of the
  buffer is stale until ``consolidate()``;
* ``w`` is a device scalar a one-thread kernel advances once per ``step()`` from two device counters
  (:attr:`counters_dev`: steps, updates; :attr:`weight_dev`), before the step's first EMA launch: eager and captured
  steps issue the same launches and a replayed graph needs no host write.  ``every=K`` updates on every K-th step
  with ``decay ** K`` (the other steps' launches return after one scalar load); ``warmup`` uses
  ``min(decay, (1 + u) / (10 + u))`` at update ``u``.  On the CPU the counters are host integers and the update is
  ``Tensor.lerp_`` parameter by parameter;
* :meth:`applied` swaps the average into the model for evaluation and checkpoints.

Limitation: buffers (the BatchNorm running statistics) are not averaged; evaluation under :meth:`applied` uses the
model's current ones.
"""
from __future__ import annotations

from collections import OrderedDict
from contextlib import contextmanager

import torch

from ..ops.ema import ema_advance_, ema_flat_, ema_weight
from .flat import FlatOptimizer

_NAME = "ema"


class WeightEMA:
    def __init__(self, optimizer: FlatOptimizer, decay: float = 0.999, warmup: bool = False, every: int = 1):
        if not isinstance(optimizer, FlatOptimizer):
            raise ValueError("WeightEMA attaches to a ddpx.optim optimizer over a flat parameter store")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"Invalid EMA decay: {decay} (0 <= decay < 1)")
        if int(every) != every or int(every) < 1:
            raise ValueError(f"Invalid EMA interval: {every} (an integer >= 1)")
        if optimizer.ema is not None:
            raise ValueError("the optimizer already has a WeightEMA attached")
        self.optimizer = optimizer
        self.flat = optimizer.flat
        self.decay, self.warmup, self.every = float(decay), bool(warmup), int(every)
        cuda = self.flat.master.is_cuda
        self.counters_dev = torch.zeros(2, dtype=torch.int32, device=self.flat.device) if cuda else None
        self.weight_dev = torch.zeros((), dtype=torch.float32, device=self.flat.device) if cuda else None
        self._host = [0, 0]  # (steps, updates) on the CPU
        self.reset()
        optimizer.ema = self

    # ------------------------------------------------------------------ state
    @property
    def buffer(self) -> torch.Tensor:
        """The average, flat and laid out like ``flat.master`` (looked up on every use: a re-layout replaces it)."""
        return self.flat.state_tensors[_NAME]

    @torch.no_grad()
    def reset(self):
        """Make the average a copy of the current weights (the counters stay)."""
        t = self.flat.state_tensors.get(_NAME)
        if t is None or t.shape != self.flat.master.shape:
            self.flat.state_tensors[_NAME] = self.flat.master.detach().clone()
        else:
            t.copy_(self.flat.master)

    def counts(self):
        """(steps, updates) so far; on the GPU read from the device counters (synchronises)."""
        if self.counters_dev is not None:
            s, u = self.counters_dev.tolist()
            return int(s), int(u)
        return tuple(self._host)

    def _set_counts(self, steps: int, updates: int):
        self._host = [int(steps), int(updates)]
        if self.counters_dev is not None:
            self.counters_dev.copy_(torch.tensor(self._host, dtype=torch.int32))

    # ------------------------------------------------------------------ the step driver's hook
    def after_updates(self, ranges):
        """Advance the counters once, then move the average towards the weights over ``ranges`` (flat [start, end)
        pairs).  Called by ``FlatOptimizer._run`` after a step's updates, on their stream."""
        f, e = self.flat, self.buffer
        if self.counters_dev is not None:
            ema_advance_(self.counters_dev, self.decay, self.warmup, self.every, self.weight_dev)
            for (s, t) in ranges:
                ema_flat_(e[s:t], f.master[s:t], self.weight_dev)
            return
        self._host[0] += 1
        self._host[1], w = ema_weight(self._host[0], self._host[1], self.decay, self.warmup, self.every)
        if w == 0.0:
            return
        for (s, t) in ranges:
            for o, n in zip(f.offsets, f.numels):  # parameter by parameter (the padding between them stays 0)
                lo, hi = max(o, s), min(o + n, t)
                if lo < hi:
                    ema_flat_(e[lo:hi], f.master[lo:hi], w)

    # ------------------------------------------------------------------ using the average
    @contextmanager
    def applied(self):
        """The model computes with the averaged weights inside the block: the contents of the master and of the
        average are swapped on entry and swapped back on exit, each time followed by ``flat.refresh_shadow()`` (the
        bf16 copy; the fp8 and conv-layout copies are re-derived by their next reader).  ``evaluate()`` and
        ``model_state_dict()`` inside see the average.  Collective under ZeRO-1 (``consolidate()`` runs first);
        not to be used during graph capture.  Buffers are not averaged."""
        f = self.flat
        if f.master.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEMA.applied() must not be used during graph capture")
        sink = f.sink
        if sink is not None and hasattr(sink, "consolidate"):
            sink.consolidate()
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    @torch.no_grad()
    def _swap(self):
        f, e = self.flat, self.buffer
        tmp = f.master.clone()
        f.master.copy_(e)
        e.copy_(tmp)
        f.refresh_shadow()

    # ------------------------------------------------------------------ (de)serialise
    def params(self) -> "OrderedDict[str, torch.Tensor]":
        """The average as {module state-dict key: tensor in parameter shape, own storage}: loads into the model
        with ``load_state_dict(..., strict=False)``.  (A sharded optimizer is consolidated first.)"""
        f, e = self.flat, self.buffer
        by_name = {f.names[id(p)]: e[f.slice(i)].view(p.shape).detach().clone() for i, p in enumerate(f.params)}
        return OrderedDict((k, by_name[k]) for k in sorted(by_name))

    def state_dict(self):
        steps, updates = self.counts()
        return {"decay": self.decay, "warmup": self.warmup, "every": self.every, "steps": steps, "updates": updates,
                "params": self.params()}

    @torch.no_grad()
    def load_state_dict(self, state):
        f, e = self.flat, self.buffer
        params = state["params"]
        missing = [f.names[id(p)] for p in f.params if f.names[id(p)] not in params]
        if missing:
            raise ValueError(f"WeightEMA.load_state_dict: no average for {missing}")
        for i, p in enumerate(f.params):
            t = params[f.names[id(p)]]
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"WeightEMA.load_state_dict: {f.names[id(p)]} has shape {tuple(t.shape)}, the "
                                 f"parameter {tuple(p.shape)}")
            e[f.slice(i)].copy_(t.reshape(-1))
        # decay / warmup / every stay as constructed (a resumed run's own options win); the counts continue
        self._set_counts(state["steps"], state["updates"])
