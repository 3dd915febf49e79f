"""LAMB (You et al., 2020): Adam moments with a layer-wise trust ratio, over the flat store.

The Adam-family counterpart of :class:`ddpx.optim.LARS` for large global batches: each parameter tensor's update
``u = m^ / (sqrt(v^) + eps) + wd w`` is scaled by ``|w| / |u|`` (the formula in :mod:`ddpx.ops.lamb`).  Biases and
BatchNorm affine parameters (``ndim <= 1``) take the same update with a ratio of 1, weight decay included, unless
``exclude_1d=False``; so does a parameter whose weight or update norm is zero or NaN.  With every ratio equal to 1
this is AdamW's update in non-decoupled form: mathematically ``torch.optim.AdamW``'s, not bitwise.

An :class:`ddpx.optim.AdamW` (its state tensors ``exp_avg`` / ``exp_avg_sq``, which follow the ZeRO-1 re-layout,
its device step counter with the two bias-correction scalars, its state dict) with another update and one more
pre-pass stage; the step driver and its schedules are :class:`ddpx.optim.flat.FlatOptimizer`'s.  What differs:

* the trust ratio needs the norm of the update itself, so a step is two streaming passes
  (``csrc/kernels/lamb.hip``).  The moments pass (``ddpx_lamb_moments``) is a pre-pass stage like LARS's norms: it
  runs per bucket as DDP's all-reduces land, or per shard as the reduce-scatters land under ZeRO-1, writes m and v
  and two partial sums (w^2, u^2) per chunk.  Then the per-parameter totals (``ddpx_lars_segment_reduce``; under
  ZeRO-1 in two spans around ONE all-reduce of the ``[2 P]`` vector, so every rank holds the same table), the
  trust table (``ddpx_lars_trust``) and the apply pass (``ddpx_lamb_apply``) range by range, each bucket's
  all-gather following its apply;
* with ``max_grad_norm`` the stages are ``[clip, moments]``: the clip stage (``GradNormPlan``) runs first, exactly
  as for AdamW: per-bucket partial sums as the collectives land and a scalar all-reduce under ZeRO-1.  The moments
  stage then waits for the clip factor, so with clipping it does NOT overlap the collectives;
* the step counter is advanced once per step, on the stream the passes run on, before the first moments launch
  (on the CPU the same hook forms the host bias corrections);
* a parameter that got no gradient in a step keeps w, m and v bit for bit in that step and its ratio reads 1;
* no update inside the backward kernels (``flat.fused_opt`` stays ``None``);
* the MX-FP8 weight copy is not written: updated ranges are marked stale and an fp8 forward re-quantises.

Parameter groups (``allow_groups=True``) may differ in ``lr``, ``weight_decay``, ``exclude_1d`` and ``adapt``
(``adapt=False``: the group keeps a ratio of 1); see :mod:`ddpx.optim.flat`.

Not implemented: a clamp of the weight norm (the paper's phi), trust clipping, ``amsgrad``.
Nobody has measured convergence with it here.
"""
from __future__ import annotations

import torch

from ..ops.lamb import LambPlan, bias_corrections
from .adamw import AdamW
from .flat import Stage


class LAMB(AdamW):
    _state_keys = {"betas": True, "exclude_1d": True}

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 1e-2,
                 exclude_1d: bool = True, capturable: bool = False, max_grad_norm: float | None = None,
                 allow_groups: bool = False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable,
                         max_grad_norm=max_grad_norm, allow_groups=allow_groups)
        # AdamW's param_group keys plus this one
        self.defaults["exclude_1d"] = bool(exclude_1d)
        for group in self.param_groups:
            group.setdefault("exclude_1d", bool(exclude_1d))
        n = len(self.flat.params)
        # per-parameter totals [w^2 x P, u^2 x P] and trust ratios of the last step (store order); the optimizer's
        # own, so the tensors stay the same whatever plan writes them
        self._sq = torch.zeros(2 * n, dtype=torch.float32, device=self.flat.device)
        self._trust = torch.ones(n, dtype=torch.float32, device=self.flat.device)
        self._bc_host = None       # the CPU path's bias corrections of the current step
        self._advance_stage = self._moments_stage()
        self._stages.append(self._advance_stage)

    def _moments_stage(self):
        def moments(plan, k):
            g = self.param_groups[0]
            plan.moments(k, self.exp_avg, self.exp_avg_sq, self._bc(), g["betas"], g["eps"], g["weight_decay"],
                         clip=self._clip, skip=self.flat.updated, hyper=self._groups_hyper())
        # which parameters adapt (the groups' exclude_1d / adapt) is part of the plan: its key
        return Stage(lambda ranges: LambPlan(self.flat, ranges, sq=self._sq, trust=self._trust, plain=self._plain),
                     moments, lambda plan: plan.trust(), key=lambda: tuple(self._plain()))

    def _groups_hyper(self):
        """The per-parameter rows when the groups differ, else None (the scalar entry points)."""
        hyper = self._hyper()
        return None if hyper.uniform else hyper

    @property
    def trust_ratio_dev(self):
        """The last step's trust ratio of every parameter, fp32 ``[P]`` on the device in store order
        (``flat.params``); 1 for the parameters that do not adapt.  Reading it on the host synchronises."""
        return self._trust

    def _bc(self):
        return self._bc_dev if self._bc_dev is not None else self._bc_host

    def _advance(self, g):
        super()._advance(g)
        if self._t_dev is None:
            self._bc_host = bias_corrections(self.step_count + 1, *g["betas"])

    @property
    def _lamb_plan(self):
        """The ``LambPlan`` of the last step (the moments stage's; None before the first)."""
        return self._advance_stage.plan

    def _update(self, start, end, g, fp8=True):
        f = self.flat
        hyper = self._groups_hyper()
        # (the CPU path steps every parameter with its group's own current rate)
        lr = self._lr_arg() if hyper is None or f.master.is_cuda else self._param_lrs(hyper)
        self._lamb_plan.apply(start, end, lr, self.exp_avg, self.exp_avg_sq, self._bc(), g["eps"],
                              g["weight_decay"], hyper=hyper)
        f.fp8_mark(start, end, False)  # this kernel does not write the MX-FP8 copy: the next reader re-quantises
