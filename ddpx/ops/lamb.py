"""LAMB over the flat store: the moments pass, the per-parameter norms, the trust table and the apply pass.

LAMB (You et al., 2020) scales each parameter tensor's Adam update by a trust ratio.  Per element, with ``gscale``
the gradient scale (the global clip factor included) and ``bc1 = 1 - beta1^t``, ``bc2s = sqrt(1 - beta2^t)``:

    g = g * gscale;  m = m + (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g g
    r = (m / bc1) / (sqrt(v) / bc2s + eps);  u = r + wd w

and for every parameter ``i`` of the store:

    wn_i = |w_i|      un_i = |u_i|                                      (fp32 device scalars)
    adapt_i = not plain_i and wn_i > 0 and un_i > 0                     (a NaN norm: False)
    t_i = wn_i / un_i  if adapt_i else 1
    w = w - (lr t_i) u

The passes (``csrc/kernels/lamb.hip``) run over :class:`ddpx.ops.lars.ParamNormPlan`'s tables: ``ddpx_lamb_moments``
writes m and v and two fp32 partials (w^2, u^2) per chunk, forming u in registers; LARS's
``ddpx_lars_segment_reduce`` and ``ddpx_lars_trust`` (with ``trust_coef = 1, weight_decay = 0, eps = 0``: exactly
``wn / un`` under the same adapt rule) produce the totals and the table; ``ddpx_lamb_apply`` recomputes u from the
stored m and v with the same device function and updates w and the bf16 shadow.  No buffer for u, no atomics and
no host read: reproducible bit for bit and graph-capturable.  No clamp of ``wn`` (the paper's phi) and no trust
clipping.

CPU tensors take a torch path over the same tables; on the CPU that path defines the semantics.
"""
from __future__ import annotations

import math

import torch

from ..runtime import native
from .lars import ParamNormPlan, _lr_args


def bias_corrections(step: int, beta1: float, beta2: float, device="cpu") -> torch.Tensor:
    """``{1 - beta1^t, sqrt(1 - beta2^t)}`` formed in fp64 and rounded once to fp32, as ``ddpx_adamw_advance``
    forms them on the device (the CPU path's ``bc``)."""
    t = int(step)
    return torch.tensor([1.0 - float(beta1) ** t, math.sqrt(1.0 - float(beta2) ** t)],
                        dtype=torch.float64).to(torch.float32).to(device)


class LambPlan(ParamNormPlan):
    """:class:`ParamNormPlan`'s chunk, segment and trust tables for LAMB over ``ranges`` of the store ``flat``,
    cached per ``(layout_version, ranges)`` as there.  ``sq`` is fp32 ``[2 P]``: w^2 totals, then u^2 totals; ``trust``
    fp32 ``[P]``.  Per step: :meth:`moments` for every range (in any order, as their gradients land),
    :meth:`reduce` (inherited; optionally in two spans around a SUM all-reduce of :attr:`sq`), :meth:`trust`, then
    :meth:`apply` for every range to step."""

    def __init__(self, flat, ranges=None, sq=None, trust=None, exclude_1d: bool = True, plain=None):
        super().__init__(flat, ranges, sq=sq, trust=trust, result=None, exclude_1d=exclude_1d, plain=plain)

    @property
    def sq_u(self):
        return self.sq[self.P:]

    def _check_states(self, m, v, what):
        p = self.flat.master
        for t in (m, v):
            if t is None or t.numel() != p.numel():
                raise ValueError(f"lamb {what}: buffers must have the store's numel")
            if t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
                raise ValueError(f"lamb {what}: the states must be contiguous fp32 tensors on the store's device")

    def moment_runs(self, k: int, skip=None):
        """``(runs, skipped)``: the runs ``[first, count]`` of range ``k``'s chunks to launch and those left out
        because their parameter is marked in ``skip`` (a bool per parameter, ``FlatParams.updated``)."""
        self._build()
        key = ("m", k, tuple(bool(s) for s in skip) if skip is not None and any(skip) else None)
        hit = self._selected.get(key)
        if hit is not None:
            return hit
        first, count = self.spans[k]
        runs, skipped = [], []
        for j in range(first, first + count):
            dst = skipped if key[2] is not None and key[2][self.chunks[j][2]] else runs
            if dst and dst[-1][0] + dst[-1][1] == j:
                dst[-1][1] += 1
            else:
                dst.append([j, 1])
        self._selected[key] = (runs, skipped)
        return runs, skipped

    def moments(self, k: int, exp_avg, exp_avg_sq, bc, betas, eps: float, weight_decay: float,
                grad_scale: float = 1.0, clip: torch.Tensor | None = None, skip=None, hyper=None):
        """The moments pass over range ``k``: m and v updated, (w^2, u^2) per chunk.  ``hyper``
        (:data:`ddpx.optim.flat.Hyper`, parameter groups): every parameter forms u with its own weight decay.  ``bc``: the fp32 ``[2]``
        bias corrections of this step (``ddpx_adamw_advance`` on the GPU, :func:`bias_corrections` on the CPU);
        ``clip``: a 0-d fp32 device factor on the gradient.  The chunks of the parameters marked in ``skip`` are
        left out (their m and v are not decayed) and their partials set to 0, so their ratio reads 1."""
        f = self.flat
        self._check_states(exp_avg, exp_avg_sq, "moments")
        if f.grad.numel() != f.master.numel():
            raise ValueError("lamb moments: buffers must have the store's numel")
        if bc is None or bc.dtype != torch.float32 or bc.numel() != 2 or bc.device != f.master.device:
            raise ValueError("lamb moments: bc must be the fp32 [2] tensor of the step's bias corrections")
        runs, skipped = self.moment_runs(k, skip)
        for (j, count) in skipped:
            self.partials_buf[j:j + count].zero_()
        if not runs:
            return
        if not f.master.is_cuda:
            self._moments_cpu(runs, exp_avg, exp_avg_sq, bc, betas, eps,
                              weight_decay if hyper is None else hyper.wd, grad_scale, clip)
            return
        if clip is not None and (clip.dtype != torch.float32 or clip.device != f.master.device):
            raise ValueError("lamb moments: clip must be an fp32 scalar on the parameters' device")
        lib = native.kernels()
        g = f.grad
        table = self._hyper_table(hyper) if hyper is not None else None
        for (j, count) in runs:
            rc = lib.ddpx_lamb_moments(f.master.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), g.data_ptr(),
                                       int(g.dtype == torch.bfloat16), self.table[j:].data_ptr(), count,
                                       native.ptr(table), self.partials_buf[j:].data_ptr(), bc.data_ptr(),
                                       float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                       float(grad_scale), native.ptr(clip), native.stream_handle())
            native.check(rc, "ddpx_lamb_moments")

    @staticmethod
    def _u(w, m, v, bc1, bc2s, eps, wd):
        return (m / bc1) / (v.sqrt() / bc2s + eps) + wd * w

    def _moments_cpu(self, runs, m, v, bc, betas, eps, wd, grad_scale, clip):
        f = self.flat
        if clip is not None:
            grad_scale = grad_scale * float(clip.item())
        w1 = float(torch.tensor(1.0 - float(betas[0]), dtype=torch.float64).float())
        w2 = float(torch.tensor(1.0 - float(betas[1]), dtype=torch.float64).float())
        b2 = float(torch.tensor(float(betas[1]), dtype=torch.float64).float())
        bc1, bc2s = float(bc[0]), float(bc[1])
        wf, gf = f.master.detach(), f.grad.detach()
        for (j, count) in runs:
            for jj in range(j, j + count):
                s, n, pid = self.chunks[jj]
                wd_ = float(wd[pid]) if isinstance(wd, (list, tuple)) else float(wd)
                g = gf[s:s + n].float()
                if grad_scale != 1.0:
                    g = g * grad_scale
                mm, vv, w = m[s:s + n], v[s:s + n], wf[s:s + n]
                mm.add_((g - mm) * w1)
                vv.mul_(b2).addcmul_(g, g, value=w2)
                u = self._u(w, mm, vv, bc1, bc2s, float(eps), wd_)
                self.partials_buf[jj, 0] = w.double().square().sum().float()
                self.partials_buf[jj, 1] = u.double().square().sum().float()

    def trust(self):
        """The trust table from ``sq``: ``wn / un`` where the parameter adapts, else 1."""
        self._trust_table(1.0, 0.0, 0.0, None)

    def compute(self, exp_avg, exp_avg_sq, bc, betas, eps, weight_decay, grad_scale: float = 1.0, clip=None,
                skip=None, hyper=None):
        """All ranges, reduce, trust (single-process use)."""
        for k in range(len(self.ranges)):
            self.moments(k, exp_avg, exp_avg_sq, bc, betas, eps, weight_decay, grad_scale, clip, skip, hyper)
        self.reduce()
        self.trust()
        return self.trust_dev

    def apply(self, start: int, end: int, lr, exp_avg, exp_avg_sq, bc, eps: float, weight_decay: float,
              hyper=None):
        """``w -= (lr t) u`` over the chunks lying in ``[start, end)``, u recomputed from the stored m and v (which,
        like the gradient, are not written); the bf16 shadow is written in the same pass.  ``lr``: a float or a
        0-d fp32 device tensor.  Padding between parameters is in no chunk and is not touched; the MX-FP8 copy is
        not written.  ``hyper`` (parameter groups): every parameter's own weight decay (the moments pass's) and, on
        the GPU, ``lr * lr_mul``; on the CPU ``lr`` is then the list of the parameters' own rates."""
        f = self.flat
        runs = self._select(int(start), int(end))
        p, sh = f.master, f.shadow
        self._check_states(exp_avg, exp_avg_sq, "apply")
        if sh is not None and sh.numel() != p.numel():
            raise ValueError("lamb apply: buffers must have the store's numel")
        if bc is None or bc.dtype != torch.float32 or bc.numel() != 2 or bc.device != p.device:
            raise ValueError("lamb apply: bc must be the fp32 [2] tensor of the step's bias corrections")
        if not p.is_cuda:
            lrs = lr if isinstance(lr, (list, tuple)) else None  # per parameter (parameter groups)
            if lrs is None:
                lr_v = float(lr) if not torch.is_tensor(lr) else float(lr.item())
            trust = self.trust_dev.tolist()
            bc1, bc2s = float(bc[0]), float(bc[1])
            pf = p.detach()
            for (j, count) in runs:
                for (s, n, pid) in self.chunks[j:j + count]:
                    w = pf[s:s + n]
                    if lrs is not None:
                        lr_v = float(lrs[pid])
                    u = self._u(w, exp_avg[s:s + n], exp_avg_sq[s:s + n], bc1, bc2s, float(eps),
                                float(weight_decay if hyper is None else hyper.wd[pid]))
                    step = float(torch.tensor(lr_v, dtype=torch.float32) * torch.tensor(trust[pid],
                                                                                       dtype=torch.float32))
                    w.add_(u, alpha=-step)
                    if sh is not None:
                        sh[s:s + n].copy_(w)
            return
        table = self._hyper_table(hyper) if hyper is not None else None
        lr_dev, lr_host = _lr_args(lr)
        lib = native.kernels()
        for (j, count) in runs:
            rc = lib.ddpx_lamb_apply(p.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), native.ptr(sh),
                                     self.table[j:].data_ptr(), count, self.trust_dev.data_ptr(), native.ptr(table),
                                     lr_dev, lr_host, bc.data_ptr(), float(eps), float(weight_decay),
                                     native.stream_handle())
            native.check(rc, "ddpx_lamb_apply")
