"""An independent fp64 LAMB, parameter by parameter, and next to it first-order bounds on the distance of an fp32
implementation from it, accumulated over the steps (shared by the LAMB tests; not a test module).  Built the way
``tests/_lars_ref.py`` is.

The reference takes the same fp32 gradients and the hyper-parameters as the kernels receive them: lr, eps, wd rounded
to fp32; w1 = fl(1 - beta1), b2 = fl(beta2), w2 = fl(1 - beta2) (1 - beta formed exactly, rounded once);
bc1 = fl(1 - beta1^t), bc2s = fl(sqrt(1 - beta2^t)) (formed in fp64, rounded once):

    c    = min(1, max_norm / (|g|_all + 1e-6))            (1 without max_norm)
    g    = c g;  m = m + (g - m) w1;  v = b2 v + w2 g g
    r    = (m / bc1) / (sqrt(v) / bc2s + eps);  u = r + wd w
    t    = |w_i| / |u_i|   if (ndim > 1 or not exclude_1d) and |w_i| > 0 and |u_i| > 0 else 1
    w    = w - (lr t) u

Bounds.  u = 2^-24 (``U``): one fp32 rounding multiplies its result by (1 + e), |e| <= U.  S = ``SUMSQ`` is the
relative bound of a sum of squares (``tests/_lars_ref.py``), ``K_M`` = 2 and ``K_V`` = 3 the roundings of AdamW's moment
updates (``tests/test_gpu_adamw.py``), ``k`` the roundings an implementation spends where the kernel has one fma
(1: the kernel; 2: the CPU path's mul + add).

* R_c, the clip factor: S + 2 u (``_lars_ref``).  E_g = c |g| (R_c + u), the scaled gradient (the factor's error and
  the product's rounding); 0 without clipping.
* m' = fma(g - m, w1, m):  E_m' = (1 - w1) E_m + w1 E_g + k K_M u (|m| + |g|).
* v' = fma(b2, v, fl(fl(g g) w2)):  E_v' = b2 E_v + 2 w2 |g| E_g + k K_V u v'  (every term >= 0).
* s = sqrt(v'):  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(b):  E_s = E_v' / sqrt(v')
  (sqrt(E_v') where v' = 0).
* den = fl(fl(s / bc2s) + eps), every term >= 0:  E_den = E_s / bc2s;  r = fl(fl(m / bc1) / den): the roundings
  sqrt, / bc2s, + eps, m / bc1 and the division, ``K_R`` = 5:
  E_r = E_m' / (bc1 den) + |r| E_den / den + K_R u |r|.
* u = fma(wd, w, r):  E_u = E_r + wd E_p + k u (|r| + wd |w|).
* t = fl(wn / un), wn = sqrt of a sum of squares within S: S / 2 + u <= S relative, and |E_p|_2 / |w|_2 from the
  implementation's own weights; un likewise with |E_u|_2 / |u|_2; the division u:
  R_t = 2 S + u + |E_p|_2 / |w|_2 + |E_u|_2 / |u|_2.
* w' = fma(-fl(lr t), u, w):  E_p' = E_p + lr t (E_u + |u| (R_t + u)) + k u (|w| + lr t |u|).

Every bound gets + 2^-149 (the smallest subnormal: an absolute rounding floor).
"""
import math

import torch

from tests._lars_ref import SUMSQ, TINY, U, f32

K_M, K_V = 2, 3  # tests/test_gpu_adamw.py
K_R = 5
K_T = 3          # a ratio from the fp32 totals the device read: two square roots and the division (1 * wn,
#                  fma(0, wn, un) and + 0 are exact)


class LambFp64:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude_1d=True,
                 max_grad_norm=None, k=1):
        self.ndim = [p.dim() for p in params]
        self.P = [p.detach().double().cpu().clone() for p in params]
        self.M = [torch.zeros_like(p) for p in self.P]
        self.V = [torch.zeros_like(p) for p in self.P]
        self.Ep = [torch.zeros_like(p) for p in self.P]
        self.Em = [torch.zeros_like(p) for p in self.P]
        self.Ev = [torch.zeros_like(p) for p in self.P]
        self.lr, self.eps, self.wd = f32(lr), f32(eps), f32(weight_decay)
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.w1, self.b2, self.w2 = f32(1.0 - self.beta1), f32(self.beta2), f32(1.0 - self.beta2)
        self.exclude_1d = exclude_1d
        self.max_norm = None if max_grad_norm is None else f32(max_grad_norm)
        self.k = k
        self.t = 0
        self.trust, self.norm, self.coef = [1.0] * len(self.P), None, 1.0
        self.Un = [0.0] * len(self.P)

    def bc(self, t):
        return f32(1.0 - self.beta1 ** t), f32(math.sqrt(1.0 - self.beta2 ** t))

    def direction(self, i, bc1, bc2s):
        """(u, E_u, |r|) of parameter i from the reference's current w, m, v and their bounds."""
        k = self.k
        W, M, V = self.P[i], self.M[i], self.V[i]
        s = V.sqrt()
        Es = torch.where(V > 0, self.Ev[i] / s.clamp_min(TINY), self.Ev[i].sqrt())
        den = s / bc2s + self.eps
        r = (M / bc1) / den
        Er = self.Em[i] / (bc1 * den) + r.abs() * (Es / bc2s) / den + K_R * U * r.abs()
        u = r + self.wd * W
        Eu = Er + self.wd * self.Ep[i] + k * U * (r.abs() + self.wd * W.abs())
        return u, Eu

    def step(self, grads, lr=None, trust=None, moments=None, scale=None, bc=None):
        """``grads[i]``: parameter i's gradient (any float dtype) or None (the parameter is skipped).  ``trust``:
        use these ratios instead of the reference's own and count no error for them.  ``moments``: ``(m, v)``
        lists to take as this step's NEW moments, exactly (the apply pass alone, given the device's m and v).
        ``scale``: a given gradient factor taken as exact (a device clip scalar) instead of ``max_norm``'s.
        ``bc``: the two fp32 bias corrections to use (the device's, read back) instead of the step count's."""
        lr = self.lr if lr is None else f32(lr)
        G = [None if g is None else g.detach().float().double().cpu() for g in grads]
        if all(g is None for g in G):
            return
        self.t += 1
        bc1, bc2s = self.bc(self.t) if bc is None else (float(bc[0]), float(bc[1]))
        c, rc = 1.0, 0.0
        if scale is not None:
            c, rc = f32(scale), 0.0
        elif self.max_norm is not None:
            self.norm = float(sum(g.square().sum() for g in G if g is not None)) ** 0.5
            c = min(1.0, self.max_norm / (self.norm + 1e-6))
            rc = SUMSQ + 2 * U
        self.coef = c
        scaled = scale is not None or self.max_norm is not None
        k = self.k
        for i, g in enumerate(G):
            if g is None:
                self.trust[i] = 1.0
                continue
            W = self.P[i]
            if moments is not None:
                self.M[i] = moments[0][i].detach().double().cpu().reshape(W.shape)
                self.V[i] = moments[1][i].detach().double().cpu().reshape(W.shape)
                self.Em[i], self.Ev[i] = torch.zeros_like(W), torch.zeros_like(W)
            else:
                gs = c * g
                Eg = gs.abs() * (rc + U) if scaled else torch.zeros_like(g)
                M, V = self.M[i], self.V[i]
                self.Em[i] = (1 - self.w1) * self.Em[i] + self.w1 * Eg + k * K_M * U * (M.abs() + gs.abs())
                self.M[i] = M + (gs - M) * self.w1
                Vn = self.b2 * V + self.w2 * gs * gs
                self.Ev[i] = self.b2 * self.Ev[i] + 2 * self.w2 * gs.abs() * Eg + k * K_V * U * Vn
                self.V[i] = Vn
            u, Eu = self.direction(i, bc1, bc2s)
            wn, un = float(W.norm()), float(u.norm())
            self.Un[i] = un
            adapt = (self.ndim[i] > 1 or not self.exclude_1d) and wn > 0 and un > 0
            if trust is not None:
                t, rt = float(trust[i]), 0.0
            elif adapt:
                t = wn / un
                rt = 2 * SUMSQ + U + float(self.Ep[i].norm()) / wn + float(Eu.norm()) / un
            else:
                t, rt = 1.0, 0.0
            self.trust[i] = t
            self.Ep[i] = self.Ep[i] + lr * t * (Eu + u.abs() * (rt + U)) + k * U * (W.abs() + lr * t * u.abs())
            self.P[i] = W - lr * t * u

    def check(self, i, p, m=None, v=None, label=""):
        """Parameter i's fp32 values against the reference within the accumulated bounds; returns the achieved
        fractions of the bounds (param, exp_avg, exp_avg_sq)."""
        out = []
        for name, got, ref, bound in (("param", p, self.P[i], self.Ep[i]), ("exp_avg", m, self.M[i], self.Em[i]),
                                      ("exp_avg_sq", v, self.V[i], self.Ev[i])):
            if got is None:
                out.append(0.0)
                continue
            got = got.detach().double().cpu().reshape(ref.shape)
            assert torch.isfinite(got).all(), (label, i, name, "non-finite")
            frac = ((got - ref).abs() / (bound + TINY)).max().item() if ref.numel() else 0.0
            assert frac <= 1.0, (label, i, name, frac)
            out.append(frac)
        return out
