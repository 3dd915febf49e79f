"""``tests/_lars_ref.py`` and ``tests/_lamb_ref.py`` with per-parameter hyper-parameters (parameter groups): independent
fp64 LARS and LAMB, parameter by parameter, with the same first-order bounds (shared by the parameter-group tests;
not a test module).

Each parameter ``i`` has its own weight decay ``wd[i]``, learning rate ``lr[i]`` and ``adapt[i]`` (False: its trust
ratio is 1 whatever its shape); everything else is those files', formula for formula, with ``wd`` and ``lr`` read
per parameter.  One term is new: ``k_lr[i]``, the roundings spent on forming the parameter's learning rate.  The CPU
path steps with each group's own rate (0); the kernels form ``lr_0 * lr_mul_i`` in fp32 (1 where ``lr_mul_i != 1``:
the product then carries a relative error of at most u, which moves the step ``lr |d'|`` by that much).  The
reference then takes ``lr[i]`` as the exact product of the two fp32 factors.
"""
import math

import torch

from tests._lamb_ref import K_M, K_R, K_V
from tests._lars_ref import SUMSQ, TINY, U, f32


def _check(pairs, i, label):
    out = []
    for name, got, ref, bound in pairs:
        if got is None:
            out.append(0.0)
            continue
        got = got.detach().double().cpu().reshape(ref.shape)
        assert torch.isfinite(got).all(), (label, i, name, "non-finite")
        frac = ((got - ref).abs() / (bound + TINY)).max().item() if ref.numel() else 0.0
        assert frac <= 1.0, (label, i, name, frac)
        out.append(frac)
    return out


class LarsGroupsFp64:
    def __init__(self, params, lr, wd, adapt, momentum=0.9, trust_coef=1e-3, eps=1e-8, exclude_1d=True,
                 nesterov=False, max_grad_norm=None, k=1, k_lr=None):
        n = len(params)
        self.ndim = [p.dim() for p in params]
        self.P = [p.detach().double().cpu().clone() for p in params]
        self.B = [torch.zeros_like(p) for p in self.P]
        self.Ep = [torch.zeros_like(p) for p in self.P]
        self.Eb = [torch.zeros_like(p) for p in self.P]
        self.lr, self.wd, self.adapt = list(lr), [f32(w) for w in wd], list(adapt)
        self.mom, self.tc, self.eps = f32(momentum), f32(trust_coef), f32(eps)
        self.exclude_1d, self.nesterov = exclude_1d, nesterov
        self.max_norm = None if max_grad_norm is None else f32(max_grad_norm)
        self.k, self.k_lr = k, list(k_lr) if k_lr is not None else [0] * n
        self.trust, self.norm, self.coef = [1.0] * n, None, 1.0

    def step(self, grads, lr=None):
        """``grads[i]``: parameter i's gradient or None (skipped); ``lr``: this step's rates per parameter."""
        lrs = self.lr if lr is None else list(lr)
        G = [None if g is None else g.detach().float().double().cpu() for g in grads]
        c, rc = 1.0, 0.0
        if self.max_norm is not None:
            self.norm = float(sum(g.square().sum() for g in G if g is not None)) ** 0.5
            c = min(1.0, self.max_norm / (self.norm + 1e-6))
            rc = SUMSQ + 2 * U
        self.coef = c
        k, mom = self.k, self.mom
        for i, g in enumerate(G):
            if g is None:
                self.trust[i] = 1.0
                continue
            W, wd, lr_i = self.P[i], self.wd[i], float(lrs[i])
            wn, gn = float(W.norm()), c * float(g.norm())
            adapt = self.adapt[i] and (self.ndim[i] > 1 or not self.exclude_1d) and wn > 0 and gn > 0
            if adapt:
                t = self.tc * wn / (gn + wd * wn + self.eps)
                rt = SUMSQ + 6 * U + (rc + U if self.max_norm is not None else 0.0) + float(self.Ep[i].norm()) / wn
            else:
                t, rt = 1.0, 0.0
            self.trust[i] = t
            A = c * g.abs() + wd * W.abs()
            D = t * (c * g + wd * W)
            Ed = t * A * (rt + rc + 3 * U) + t * wd * self.Ep[i]
            Bn = mom * self.B[i] + D
            Eb = mom * self.Eb[i] + Ed + k * U * (mom * self.B[i].abs() + D.abs())
            if self.nesterov:
                DD = D + mom * Bn
                Edd = mom * Eb + Ed + k * U * (mom * Bn.abs() + D.abs())
            else:
                DD, Edd = Bn, Eb
            self.Ep[i] = (self.Ep[i] + lr_i * Edd + k * U * (W.abs() + lr_i * DD.abs())
                          + self.k_lr[i] * U * lr_i * DD.abs())
            self.P[i] = W - lr_i * DD
            self.B[i], self.Eb[i] = Bn, Eb

    def check(self, i, p, buf, label=""):
        return _check((("param", p, self.P[i], self.Ep[i]), ("momentum", buf, self.B[i], self.Eb[i])), i, label)


class LambGroupsFp64:
    def __init__(self, params, lr, wd, adapt, betas=(0.9, 0.999), eps=1e-6, exclude_1d=True, max_grad_norm=None,
                 k=1, k_lr=None):
        n = len(params)
        self.ndim = [p.dim() for p in params]
        self.P = [p.detach().double().cpu().clone() for p in params]
        self.M = [torch.zeros_like(p) for p in self.P]
        self.V = [torch.zeros_like(p) for p in self.P]
        self.Ep = [torch.zeros_like(p) for p in self.P]
        self.Em = [torch.zeros_like(p) for p in self.P]
        self.Ev = [torch.zeros_like(p) for p in self.P]
        self.lr, self.wd, self.adapt = list(lr), [f32(w) for w in wd], list(adapt)
        self.eps = f32(eps)
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.w1, self.b2, self.w2 = f32(1.0 - self.beta1), f32(self.beta2), f32(1.0 - self.beta2)
        self.exclude_1d = exclude_1d
        self.max_norm = None if max_grad_norm is None else f32(max_grad_norm)
        self.k, self.k_lr = k, list(k_lr) if k_lr is not None else [0] * n
        self.t = 0
        self.trust, self.norm, self.coef = [1.0] * n, None, 1.0

    def bc(self, t):
        return f32(1.0 - self.beta1 ** t), f32(math.sqrt(1.0 - self.beta2 ** t))

    def step(self, grads, lr=None):
        lrs = self.lr if lr is None else list(lr)
        G = [None if g is None else g.detach().float().double().cpu() for g in grads]
        if all(g is None for g in G):
            return
        self.t += 1
        bc1, bc2s = self.bc(self.t)
        c, rc = 1.0, 0.0
        if self.max_norm is not None:
            self.norm = float(sum(g.square().sum() for g in G if g is not None)) ** 0.5
            c = min(1.0, self.max_norm / (self.norm + 1e-6))
            rc = SUMSQ + 2 * U
        self.coef = c
        scaled = self.max_norm is not None
        k = self.k
        for i, g in enumerate(G):
            if g is None:
                self.trust[i] = 1.0
                continue
            W, wd, lr_i = self.P[i], self.wd[i], float(lrs[i])
            gs = c * g
            Eg = gs.abs() * (rc + U) if scaled else torch.zeros_like(g)
            M, V = self.M[i], self.V[i]
            self.Em[i] = (1 - self.w1) * self.Em[i] + self.w1 * Eg + k * K_M * U * (M.abs() + gs.abs())
            self.M[i] = M + (gs - M) * self.w1
            Vn = self.b2 * V + self.w2 * gs * gs
            self.Ev[i] = self.b2 * self.Ev[i] + 2 * self.w2 * gs.abs() * Eg + k * K_V * U * Vn
            self.V[i] = Vn
            M, V = self.M[i], self.V[i]
            s = V.sqrt()
            Es = torch.where(V > 0, self.Ev[i] / s.clamp_min(TINY), self.Ev[i].sqrt())
            den = s / bc2s + self.eps
            r = (M / bc1) / den
            Er = self.Em[i] / (bc1 * den) + r.abs() * (Es / bc2s) / den + K_R * U * r.abs()
            u = r + wd * W
            Eu = Er + wd * self.Ep[i] + k * U * (r.abs() + wd * W.abs())
            wn, un = float(W.norm()), float(u.norm())
            adapt = self.adapt[i] and (self.ndim[i] > 1 or not self.exclude_1d) and wn > 0 and un > 0
            if adapt:
                t = wn / un
                rt = 2 * SUMSQ + U + float(self.Ep[i].norm()) / wn + float(Eu.norm()) / un
            else:
                t, rt = 1.0, 0.0
            self.trust[i] = t
            self.Ep[i] = (self.Ep[i] + lr_i * t * (Eu + u.abs() * (rt + U)) + k * U * (W.abs() + lr_i * t * u.abs())
                          + self.k_lr[i] * U * lr_i * t * u.abs())
            self.P[i] = W - lr_i * t * u

    def check(self, i, p, m=None, v=None, label=""):
        return _check((("param", p, self.P[i], self.Ep[i]), ("exp_avg", m, self.M[i], self.Em[i]),
                       ("exp_avg_sq", v, self.V[i], self.Ev[i])), i, label)
