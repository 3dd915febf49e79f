"""LAMB (You et al., 2020): Adam moments with a layer-wise trust ratio, over the flat store.

The Adam-family counterpart of :class:`ddpx.optim.LARS` for large global batches: each parameter tensor's update
``u = m^ / (sqrt(v^) + eps) + wd w`` is scaled by ``|w| / |u|`` (the formula in :mod:`ddpx.ops.lamb`).  Biases and
BatchNorm affine parameters (``ndim <= 1``) take the same update with a ratio of 1, weight decay included, unless
``exclude_1d=False``; so does a parameter whose weight or update norm is zero or NaN.  With every ratio equal to 1
this is AdamW's update in non-decoupled form: mathematically ``torch.optim.AdamW``'s, not bitwise.

Built on :class:`ddpx.optim.AdamW`: the state tensors ``exp_avg`` / ``exp_avg_sq`` (which follow the ZeRO-1
re-layout), the device step counter with its two bias-correction scalars, and the rule that a step in which no
parameter had a gradient does not count.  Everything around the update rule is :class:`ddpx.optim.SGD`'s: the
whole-store step, the per-bucket steps that overlap DDP's all-reduces (compute or side stream), the ZeRO-1 shard
steps (current or communicator stream), the device LR scalar / table and HIP-graph capture.  What differs:

* the trust ratio needs the norm of the update itself, so a step is two streaming passes
  (``csrc/kernels/lamb.hip``).  The moments pass (``ddpx_lamb_moments``) takes the place LARS's norm pass has: it
  runs per bucket as DDP's all-reduces land, or per shard as the reduce-scatters land under ZeRO-1, writes m and v
  and two partial sums (w^2, u^2) per chunk.  Then the per-parameter totals (``ddpx_lars_segment_reduce``; under
  ZeRO-1 in two spans around ONE all-reduce of the ``[2 P]`` vector, so every rank holds the same table), the
  trust table (``ddpx_lars_trust``) and the apply pass (``ddpx_lamb_apply``) range by range, each bucket's
  all-gather following its apply;
* with ``max_grad_norm`` the SGD class's clip pass (``GradNormPlan``) runs first, exactly as it is: per-bucket
  partial sums as the collectives land and a scalar all-reduce under ZeRO-1.  The moments pass then waits for the
  clip factor, so with clipping it does NOT overlap the collectives;
* the step counter is advanced once per step, on the stream the passes run on, before the first moments launch;
* a parameter that got no gradient in a step keeps w, m and v bit for bit in that step and its ratio reads 1;
* no update inside the backward kernels (``flat.fused_opt`` stays ``None``);
* the MX-FP8 weight copy is not written: updated ranges are marked stale and an fp8 forward re-quantises.

Not implemented: a clamp of the weight norm (the paper's phi), trust clipping, per-group exclusions, ``amsgrad``.
Nobody has measured convergence with it here.
"""
from __future__ import annotations

import torch

from ..ops.elementwise import adamw_advance_
from ..ops.lamb import LambPlan, bias_corrections
from .adamw import AdamW


class _StepPlan(LambPlan):
    """The plan as ``SGD.step`` drives it: its ``partials(k)`` is the optimizer's moments pass over range k."""
    opt = None

    def partials(self, k: int = 0):
        self.opt._moments(self, k)


class LAMB(AdamW):
    _lamb_state = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 1e-2,
                 exclude_1d: bool = True, capturable: bool = False, max_grad_norm: float | None = None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable,
                         max_grad_norm=max_grad_norm)
        # AdamW's param_group keys plus this one
        self.defaults["exclude_1d"] = bool(exclude_1d)
        self.param_groups[0]["exclude_1d"] = bool(exclude_1d)
        n = len(self.flat.params)
        # per-parameter totals [w^2 x P, u^2 x P] and trust ratios of the last step (store order); the optimizer's
        # own, so the tensors stay the same whatever plan writes them
        self._sq = torch.zeros(2 * n, dtype=torch.float32, device=self.flat.device)
        self._trust = torch.ones(n, dtype=torch.float32, device=self.flat.device)
        self._lamb_plan = None
        self._phase = "lamb"       # "clip" while a clipped step runs the SGD class's norm pass
        self._in_sharded = False
        self._bc_host = None       # the CPU path's bias corrections of the current step

    @property
    def trust_ratio_dev(self):
        """The last step's trust ratio of every parameter, fp32 ``[P]`` on the device in store order
        (``flat.params``); 1 for the parameters that do not adapt.  Reading it on the host synchronises."""
        return self._trust

    def _bc(self):
        return self._bc_dev if self._bc_dev is not None else self._bc_host

    # ------------------------------------------------------------------ the passes SGD.step drives
    def _pre_pass_needed(self) -> bool:
        return True

    def _plan(self, ranges):
        if self._phase == "clip":
            return super()._plan(ranges)  # the SGD class's GradNormPlan (self._norm_plan)
        ranges = [(int(a), int(b)) for a, b in ranges]
        pl = self._lamb_plan
        ex = bool(self.param_groups[0]["exclude_1d"])
        if pl is None or pl.ranges != ranges or pl.exclude_1d != ex:
            pl = self._lamb_plan = _StepPlan(self.flat, ranges, sq=self._sq, trust=self._trust, exclude_1d=ex)
            pl.opt = self
        return pl

    def _moments(self, plan, k):
        g = self.param_groups[0]
        skip = self.flat.updated
        if self._advance_due and not all(skip):
            # once per step, on the stream the step's passes run on, before the first moments launch (decided
            # from the whole store, so every rank of a sharded run advances in the same steps)
            self._advance_due = False
            if self._t_dev is not None:
                adamw_advance_(self._t_dev, self._bc_dev, *g["betas"])
            else:
                self._bc_host = bias_corrections(self.step_count + 1, *g["betas"])
        plan.moments(k, self.exp_avg, self.exp_avg_sq, self._bc(), g["betas"], g["eps"], g["weight_decay"],
                     clip=self._clip, skip=skip)

    def _pre_finish(self, plan):
        if self._phase == "clip":
            super()._pre_finish(plan)  # the clip factor; self._clip
            self._phase = "lamb"
            if self._in_sharded:
                return  # _sharded_norm runs the LAMB sequence itself, around its own all-reduce
            lp = self._plan(plan.ranges)
            for k in range(len(lp.ranges)):
                lp.partials(k)
            lp.reduce()
            plan = lp
        plan.trust()

    def _sharded_norm(self, src, order, wait):
        if self._phase == "clip":
            self._in_sharded = True
            try:
                super()._sharded_norm(src, order, wait)  # scalar all-reduce, clip factor
            finally:
                self._in_sharded = False
            wait = lambda b: None  # noqa: E731 - every bucket has landed
        super()._sharded_norm(src, order, wait)  # moments per shard, [2 P] all-reduce, trust table

    def _update(self, start, end, g, fp8=True):
        if self._advance_due:
            return  # no moments launch this step: nothing has a gradient, nothing to apply
        f = self.flat
        self._lamb_plan.apply(start, end, self._lr_arg(), self.exp_avg, self.exp_avg_sq, self._bc(), g["eps"],
                              g["weight_decay"])
        f.fp8_mark(start, end, False)  # this kernel does not write the MX-FP8 copy: the next reader re-quantises

    @torch.no_grad()
    def step(self, closure=None):
        self._phase = "clip" if self.max_grad_norm is not None else "lamb"
        try:
            return super().step(closure)
        finally:
            self._phase = "lamb"

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._lamb_plan = None  # (exclude_1d may have changed)
