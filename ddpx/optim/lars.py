"""LARS (You et al., 2017): momentum SGD with a layer-wise trust ratio, fused into the flat update.

For large global batches: each parameter tensor's update is scaled by ``trust_coef * |w| / (|g| + wd |w| + eps)``
(the formula, with clipping, in :mod:`ddpx.ops.lars`).  Biases and BatchNorm affine parameters (``ndim <= 1``) keep
plain SGD, weight decay included, unless ``exclude_1d=False``; so does a parameter whose weight or gradient norm is
zero or NaN.

A :class:`ddpx.optim.SGD` (its ``momentum`` state and state dict) with another update and its own pre-pass; the
step driver and its schedules are :class:`ddpx.optim.flat.FlatOptimizer`'s.  What differs from SGD:

* its one pre-pass stage always runs, and computes per-parameter sums of w^2 and g^2 (``ddpx_lars_sumsq`` +
  ``ddpx_lars_segment_reduce``) and the trust table (``ddpx_lars_trust``).  It replaces SGD's clip stage: with
  ``max_grad_norm`` the global norm and clip factor come out of the same sums, so the gradient is still read once
  before the update.  Under ZeRO-1 each rank sums over its own pieces of master and gradient and ONE
  all-reduce of the ``[2 P]`` vector completes the totals, so every rank holds the same trust table;
* the update is ``ddpx_sgd_flat_chunks`` (``csrc/kernels/lars.hip``), driven by the pass's chunk table.  A trust
  ratio of exactly 1 gives ``ddpx_sgd_flat``'s bits;
* no update inside the backward kernels: LARS needs the materialised gradient (``flat.fused_opt`` stays ``None``);
* the MX-FP8 weight copy is not written: updated ranges are marked stale and an fp8 forward re-quantises.

Parameter groups (``allow_groups=True``) may differ in ``lr``, ``weight_decay``, ``exclude_1d`` and ``adapt``
(``adapt=False``: the group keeps plain SGD); see :mod:`ddpx.optim.flat`.  No trust clipping (LARC).
"""
from __future__ import annotations

import torch

from .flat import FlatOptimizer, Stage
from .sgd import SGD


class LARS(SGD):
    _state_keys = {"momentum": True, "trust_coef": True}

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 0.0,
                 trust_coef: float = 1e-3, eps: float = 1e-8, exclude_1d: bool = True, nesterov: bool = False,
                 capturable: bool = False, max_grad_norm: float | None = None, allow_groups: bool = False):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not float(trust_coef) > 0:
            raise ValueError(f"Invalid trust_coef value: {trust_coef}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        # SGD's param_group keys plus the three LARS ones
        FlatOptimizer.__init__(self, params, dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay,
                                                  nesterov=nesterov, trust_coef=float(trust_coef), eps=float(eps),
                                                  exclude_1d=bool(exclude_1d)),
                               capturable, False, max_grad_norm, states=("momentum",), allow_groups=allow_groups)
        n = len(self.flat.params)
        # per-parameter totals [w^2 x P, g^2 x P] and trust ratios of the last step (store order); the optimizer's
        # own, so the tensors stay the same whatever plan writes them
        self._sq = torch.zeros(2 * n, dtype=torch.float32, device=self.flat.device)
        self._trust = torch.ones(n, dtype=torch.float32, device=self.flat.device)
        self._stages = [self._lars_stage()]

    def _lars_stage(self):
        from ..ops.lars import LarsPlan

        def finish(plan):
            g = self.param_groups[0]
            hyper = self._hyper()
            plan.trust(g["trust_coef"], g["weight_decay"], g["eps"], self.max_grad_norm,
                       hyper=None if hyper.uniform else hyper)
            self._clip = plan.coef_dev if self.max_grad_norm is not None else None
        # which parameters adapt (the groups' exclude_1d / adapt) is part of the plan: its key
        return Stage(lambda ranges: LarsPlan(self.flat, ranges, sq=self._sq, trust=self._trust,
                                             result=self._clip_res, plain=self._plain),
                     lambda plan, k: plan.partials(k), finish, key=lambda: tuple(self._plain()))

    @property
    def trust_ratio_dev(self):
        """The last step's trust ratio of every parameter, fp32 ``[P]`` on the device in store order
        (``flat.params``); 1 for the parameters that kept plain SGD.  Reading it on the host synchronises."""
        return self._trust

    @property
    def _norm_plan(self):
        """The ``LarsPlan`` of the last step (its stage's; None before the first)."""
        return self._stages[0].plan

    def _update(self, start, end, g, fp8=True):
        f = self.flat
        hyper = self._hyper()
        if hyper.uniform:
            hyper, lr = None, self._lr_arg()
        else:  # the CPU path steps every parameter with its group's own current rate
            lr = self._lr_arg() if f.master.is_cuda else self._param_lrs(hyper)
        self._norm_plan.update(start, end, lr, g["momentum"], g["weight_decay"], nesterov=g["nesterov"],
                               clip=self._clip, momentum_buf=self.momentum_buffer, hyper=hyper)
        f.fp8_mark(start, end, False)  # this kernel does not write the MX-FP8 copy: the next reader re-quantises
