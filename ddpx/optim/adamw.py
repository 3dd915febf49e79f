"""Fused flat-buffer AdamW (decoupled weight decay) — drop-in for torch.optim.AdamW.

Everything around the update rule is :class:`ddpx.optim.flat.FlatOptimizer`'s: the whole-store step, the
per-bucket steps that overlap DDP's all-reduces (compute or side stream), the ZeRO-1 shard steps (current or
communicator stream), global-norm clipping, the device LR scalar / table and HIP-graph capture.  This module adds:

* the update is ``ddpx_adamw_flat`` (``csrc/kernels/adamw.hip``): one streaming pass over p, exp_avg,
  exp_avg_sq and the gradient, 30 B per weight (28 with bf16 gradients), bf16 shadow written in the same pass;
* two state tensors, ``flat.state_tensors["exp_avg"]`` / ``["exp_avg_sq"]``, which the sharded re-layout, the
  consolidation before a checkpoint and the state dict carry like SGD's momentum;
* a step counter.  On the GPU it is a device int32 that a one-thread kernel advances once per step (the driver's
  ``_advance`` hook: before the step's first update launch, on its stream); the same kernel writes the two
  bias-correction scalars every update launch of the step reads.  Eager and captured steps issue the same launches
  and a replayed graph needs no host write.  On the CPU the count is the host's ``step_count``.  A step in which
  no parameter had a gradient launches nothing and does not count;
* no update inside the backward kernels: AdamW needs the materialised gradient (``flat.fused_opt`` stays
  ``None``), the path ``--no_fused_optimizer`` and clipping take;
* the MX-FP8 weight copy is not written: updated ranges are marked stale and an fp8 forward re-quantises.

Limitation: ONE global step count.  A parameter that got no gradient in a step is left untouched in that step,
as in torch, but its bias correction afterwards follows the global count, not a per-parameter one.
"""
from __future__ import annotations

import torch

from ..ops.elementwise import adamw_advance_, adamw_flat_
from .flat import FlatOptimizer

_STATES = ("exp_avg", "exp_avg_sq")


class AdamW(FlatOptimizer):
    _state_keys = {"betas": True, "exclude_1d": False}

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, maximize: bool = False, capturable: bool = False,
                 max_grad_norm: float | None = None, allow_groups: bool = False):
        if amsgrad:
            raise ValueError("ddpx.optim.AdamW implements amsgrad=False")
        if maximize:
            raise ValueError("ddpx.optim.AdamW implements maximize=False")
        betas = (float(betas[0]), float(betas[1]))
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # torch.optim.AdamW's param_group keys, in its order: state_dict() is interchangeable with torch's
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=bool(capturable),
                                      differentiable=False, fused=None, decoupled_weight_decay=True),
                         capturable, False, max_grad_norm, states=_STATES, allow_groups=allow_groups)
        cuda = self.flat.master.is_cuda
        # device step counter t and {1 - beta1^t, sqrt(1 - beta2^t)} (ddpx_adamw_advance); the optimizer's own,
        # not the store's: scalars, the same on every rank
        self._t_dev = torch.zeros(1, dtype=torch.int32, device=self.flat.device) if cuda else None
        self._bc_dev = torch.ones(2, dtype=torch.float32, device=self.flat.device) if cuda else None

    @property
    def exp_avg(self):
        return self.flat.state_tensors["exp_avg"]

    @property
    def exp_avg_sq(self):
        return self.flat.state_tensors["exp_avg_sq"]

    @property
    def step_dev(self):
        """The device step counter (int32 [1]; None on the CPU): the number of steps taken."""
        return self._t_dev

    def steps_taken(self) -> int:
        """Steps taken so far; on the GPU read from the device counter (synchronises)."""
        return int(self._t_dev.item()) if self._t_dev is not None else int(self.step_count)

    def _update(self, start, end, g, fp8=True):
        f = self.flat
        hyper = self._hyper()
        if not hyper.uniform:
            self._update_groups(start, end, g, hyper)
            return
        sh = f.shadow[start:end] if f.shadow is not None else None
        adamw_flat_(f.master[start:end], self.exp_avg[start:end], self.exp_avg_sq[start:end], f.grad[start:end], sh,
                    self._lr_arg(), self._bc_dev, self.step_count + 1, g["betas"][0], g["betas"][1], g["eps"],
                    g["weight_decay"], clip=self._clip)
        f.fp8_mark(start, end, False)  # this kernel does not write the MX-FP8 copy: the next reader re-quantises

    def _update_groups(self, start, end, g, hyper):
        """The step with parameter groups that differ.  GPU: ``ddpx_adamw_flat_hyper`` over the schedule's chunk
        table (group 0's lr times each parameter's multiplier).  CPU: the scalar update parameter by parameter with
        its group's own current lr and weight decay, torch.optim.AdamW's bits."""
        f = self.flat
        if f.master.is_cuda:
            self._update_plan().adamw_update(start, end, hyper, self._lr_arg(), self.exp_avg, self.exp_avg_sq,
                                             self._bc_dev, g["betas"][0], g["betas"][1], g["eps"], clip=self._clip)
        else:
            lrs = self._param_lrs(hyper)
            for i, (o, n) in enumerate(zip(f.offsets, f.numels)):
                lo, hi = max(o, start), min(o + n, end)
                if lo < hi:
                    sh = f.shadow[lo:hi] if f.shadow is not None else None
                    adamw_flat_(f.master[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], f.grad[lo:hi], sh,
                                lrs[i], None, self.step_count + 1, g["betas"][0], g["betas"][1], g["eps"],
                                hyper.wd[i], clip=self._clip)
        f.fp8_mark(start, end, False)

    def _advance(self, g):
        if self._t_dev is not None:
            adamw_advance_(self._t_dev, self._bc_dev, *g["betas"])

    # ------------------------------------------------------- (de)serialise
    def state_dict(self):
        """torch.optim.AdamW's format: per parameter {"step", "exp_avg", "exp_avg_sq"} in parameter shape (a
        sharded optimizer is consolidated first, ``DistributedDataParallel.consolidate``)."""
        sd = super().state_dict()
        t = self.steps_taken()
        state = {}
        if t > 0:
            m, v = self.exp_avg, self.exp_avg_sq
            for i, p in enumerate(self._all_params()):
                sl = self.flat.slice(self.flat.index[id(p)])
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32),
                            "exp_avg": m[sl].view(p.shape).clone(),
                            "exp_avg_sq": v[sl].view(p.shape).clone()}
        sd["state"] = state
        sd["ddpx_step_count"] = t
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        st = state_dict.pop("state", {})
        groups = state_dict["param_groups"]
        self._check_state_kind(groups)
        if any(gr.get("amsgrad") or gr.get("maximize") for gr in groups):
            raise ValueError("ddpx.optim.AdamW implements amsgrad=False, maximize=False")
        params = self._all_params()
        self._load_groups(groups, skip=("capturable",))
        steps = set()
        m, v = self.exp_avg, self.exp_avg_sq
        for i, p in enumerate(params):
            s = st.get(i, st.get(str(i)))
            sl = self.flat.slice(self.flat.index[id(p)])
            if s is None:
                m[sl].zero_()
                v[sl].zero_()
                continue
            if "exp_avg" not in s or "exp_avg_sq" not in s:
                raise ValueError("ddpx.optim.AdamW.load_state_dict: parameter state without exp_avg / exp_avg_sq")
            m[sl].copy_(s["exp_avg"].reshape(-1))
            v[sl].copy_(s["exp_avg_sq"].reshape(-1))
            steps.add(int(float(s["step"])))
        if len(steps) > 1:
            raise ValueError(f"ddpx.optim.AdamW keeps one global step count; the state has {sorted(steps)}")
        t = steps.pop() if steps else int(state_dict.get("ddpx_step_count", 0))
        self.step_count = t
        if self._t_dev is not None:
            self._t_dev.fill_(t)
        self._state_loaded()
