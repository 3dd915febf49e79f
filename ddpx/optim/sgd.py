"""Fused flat-buffer SGD (momentum, weight decay) — drop-in for torch.optim.SGD.

Reference: ``torch.optim.SGD(model.parameters(), lr=0.4, momentum=0.9, weight_decay=5e-4)`` in the reference's
``singlegpu.py`` (default foreach path, ``torch/optim/sgd.py``: 4 multi-tensor passes / step).

Here all parameters are views of one flat fp32 buffer (``FlatParams``), so a step is ONE kernel launch
(``ddpx_sgd_flat``) that reads p, g, momentum once and writes p, momentum and the bf16 compute shadow (and the
MX-FP8 copy of a store that keeps one) once.  This module is that update rule, the ``momentum`` state tensor and
its state dict; with ``fused_backward`` the same update runs inside the kernels that produce the gradients.

Everything around the rule is :class:`ddpx.optim.flat.FlatOptimizer`'s: the binding to the store, the device LR
scalar / table (``capturable=True`` makes ``step()`` safe inside a HIP graph), global-norm clipping as a pre-pass
stage, and the step driver with its schedules (whole store, one launch per DDP bucket as its all-reduce lands,
ZeRO-1 shards).  It subclasses ``torch.optim.Optimizer``, so torch LR schedulers (``LambdaLR``) drive it unchanged.
"""
from __future__ import annotations

from ..ops.elementwise import sgd_flat_
from .flat import FlatOptimizer, take_lr_advance  # noqa: F401 - imported from here by the models and the benchmark


class SGD(FlatOptimizer):
    _state_keys = {"momentum": True, "trust_coef": False}

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, capturable: bool = False,
                 fused_backward: bool = False, max_grad_norm: float | None = None, allow_groups: bool = False):
        if dampening != 0.0:
            raise ValueError("ddpx.optim.SGD implements dampening=0 (the reference's setting)")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov), capturable, bool(fused_backward and not nesterov),
                         max_grad_norm, states=("momentum",) if momentum else (), allow_groups=allow_groups)

    @property
    def momentum_buffer(self):
        return self.flat.state_tensors.get("momentum")

    def _update(self, start, end, g, fp8=True):
        f = self.flat
        hyper = self._hyper()
        if not hyper.uniform:
            self._update_groups(start, end, g, hyper)
            return
        buf = self.momentum_buffer[start:end] if self.momentum_buffer is not None else f.master[start:end]
        sh = f.shadow[start:end] if f.shadow is not None else None
        # a store that keeps an MX-FP8 weight copy gets it written in the same pass (fp8 forward GEMMs)
        mx8 = f.mx8_range(start, end) if (fp8 and f.master.is_cuda) else None
        sgd_flat_(f.master[start:end], buf, f.grad[start:end], sh, self._lr_arg(), g["momentum"],
                  g["weight_decay"], nesterov=g["nesterov"], mx8=mx8, clip=self._clip)
        f.fp8_mark(start, end, mx8 is not None)

    def _update_groups(self, start, end, g, hyper):
        """The step with parameter groups that differ.  GPU: ``ddpx_sgd_flat_chunks`` over the schedule's chunk
        table (group 0's lr times each parameter's multiplier; the MX-FP8 copy is not written, the range is marked
        stale).  CPU: the scalar update parameter by parameter with its group's own current lr and weight decay,
        torch.optim.SGD's bits."""
        f = self.flat
        if f.master.is_cuda:
            self._update_plan().sgd_update(start, end, hyper, self._lr_arg(), g["momentum"], nesterov=g["nesterov"],
                                           clip=self._clip, momentum_buf=self.momentum_buffer)
            f.fp8_mark(start, end, False)
            return
        lrs = self._param_lrs(hyper)
        for i, (o, n) in enumerate(zip(f.offsets, f.numels)):
            lo, hi = max(o, start), min(o + n, end)
            if lo < hi:
                buf = self.momentum_buffer[lo:hi] if self.momentum_buffer is not None else f.master[lo:hi]
                sh = f.shadow[lo:hi] if f.shadow is not None else None
                sgd_flat_(f.master[lo:hi], buf, f.grad[lo:hi], sh, lrs[i], g["momentum"], hyper.wd[i],
                          nesterov=g["nesterov"], clip=self._clip)

    # ------------------------------------------------------- (de)serialise
    def state_dict(self):
        sd = super().state_dict()
        state = {}
        if self.momentum_buffer is not None and self.step_count > 0:
            for i, p in enumerate(self._all_params()):
                j = self.flat.index[id(p)]
                state[i] = {"momentum_buffer": self.momentum_buffer[self.flat.slice(j)].view(p.shape).clone()}
        sd["state"] = state
        sd["ddpx_step_count"] = self.step_count
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        st = state_dict.pop("state", {})
        self.step_count = int(state_dict.pop("ddpx_step_count", 0))
        groups = state_dict["param_groups"]
        self._check_state_kind(groups)
        self._load_groups(groups)
        if self.momentum_buffer is not None:
            for i, p in enumerate(self._all_params()):
                s = st.get(i, st.get(str(i)))
                if s is not None and s.get("momentum_buffer") is not None:
                    j = self.flat.index[id(p)]
                    self.momentum_buffer[self.flat.slice(j)].copy_(s["momentum_buffer"].reshape(-1))
        self._state_loaded()
