"""An independent fp64 LARS, parameter by parameter, and next to it first-order bounds on the distance of an fp32
implementation from it, accumulated over the steps (shared by the LARS tests; not a test module).

The reference takes the same fp32 gradients and the hyper-parameters rounded to fp32, as the kernels receive them:

    c    = min(1, max_norm / (|g|_all + 1e-6))            (1 without max_norm)
    wn   = |w_i|    gn = c |g_i|
    t    = trust_coef wn / (gn + wd wn + eps)   if (ndim > 1 or not exclude_1d) and wn > 0 and gn > 0 else 1
    d    = t (c g + wd w);  buf = mom buf + d;  d' = d + mom buf if nesterov else buf;  w -= lr d'

Bounds.  u = 2^-24: one fp32 rounding multiplies its result by (1 + e), |e| <= u.  S = ``SUMSQ`` is the relative
bound of a sum of squares (``tests/test_gpu_clip.py``'s BOUND: 44 u, every term >= 0), ``k`` the roundings an
implementation spends where the kernel has one fma (1: the kernel; 2: the CPU path's mul + add).

* R_c, the clip factor: the norm is sqrt of a sum within S (S / 2 + u <= S), + 1e-6 and the division: S + 2 u.
* R_t, a trust ratio.  wn = sqrt(sq_w): S / 2 + u.  gn = c sqrt(sq_g): S / 2 + u, and R_c + u when clipped.
  trust_coef * wn: + u.  The denominator fma(wd, wn, gn) + eps has only terms >= 0, so its relative error is at most
  its inputs' larger one + 2 u (the fma, the add); the division: + u.  In all R_t0 = S + 6 u (+ R_c + u).  The
  implementation's weights are E_p away from the reference's, which moves wn by at most |E_p|_2 / |w|_2 relatively and
  t by no more (t = trust_coef / (gn / wn + wd + eps / wn) is less than linear in wn): R_t = R_t0 + |E_p|_2 / |w|_2.
* d = fl(t fl(fma(wd, w, fl(g gscale)))): three roundings of quantities bounded by A = c |g| + wd |w|, and the
  errors of c, t and w:  E_d = t A (R_t + R_c + 3 u) + t wd E_p.
* buf' = fma(mom, buf, d):  E_b' = mom E_b + E_d + k u (mom |buf| + |d|).
* nesterov, d' = fma(mom, buf', d):  E_d' = mom E_b' + E_d + k u (mom |buf'| + |d|);  else E_d' = E_b'.
* w' = fma(-lr, d', w):  E_p' = E_p + lr E_d' + k u (|w| + lr |d'|).

Every bound gets + 2^-149 (the smallest subnormal: an absolute rounding floor).
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
SUMSQ = (33 + 2 + 6 + 2 + 1) * U  # tests/test_gpu_clip.py BOUND


def f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


class LarsFp64:
    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, trust_coef=1e-3, eps=1e-8, exclude_1d=True,
                 nesterov=False, max_grad_norm=None, k=1):
        self.ndim = [p.dim() for p in params]
        self.P = [p.detach().double().cpu().clone() for p in params]
        self.B = [torch.zeros_like(p) for p in self.P]
        self.Ep = [torch.zeros_like(p) for p in self.P]
        self.Eb = [torch.zeros_like(p) for p in self.P]
        self.lr, self.mom, self.wd = f32(lr), f32(momentum), f32(weight_decay)
        self.tc, self.eps = f32(trust_coef), f32(eps)
        self.exclude_1d, self.nesterov = exclude_1d, nesterov
        self.max_norm = None if max_grad_norm is None else f32(max_grad_norm)
        self.k = k
        self.trust, self.norm, self.coef = [1.0] * len(self.P), None, 1.0

    def step(self, grads, lr=None, trust=None):
        """``grads[i]``: parameter i's gradient (any float dtype) or None (the parameter is skipped).  ``trust``:
        use these ratios instead of the reference's own and count no error for them (one kernel launch given a
        trust table)."""
        lr = self.lr if lr is None else f32(lr)
        G = [None if g is None else g.detach().float().double().cpu() for g in grads]
        c, rc = 1.0, 0.0
        if self.max_norm is not None:
            self.norm = float(sum(g.square().sum() for g in G if g is not None)) ** 0.5
            c = min(1.0, self.max_norm / (self.norm + 1e-6))
            rc = SUMSQ + 2 * U
        self.coef = c
        k, mom, wd = self.k, self.mom, self.wd
        for i, g in enumerate(G):
            if g is None:
                self.trust[i] = 1.0
                continue
            W = self.P[i]
            wn, gn = float(W.norm()), c * float(g.norm())
            adapt = (self.ndim[i] > 1 or not self.exclude_1d) and wn > 0 and gn > 0
            if trust is not None:
                t, rt = float(trust[i]), 0.0
            elif adapt:
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
            self.Ep[i] = self.Ep[i] + lr * Edd + k * U * (W.abs() + lr * DD.abs())
            self.P[i] = W - lr * DD
            self.B[i], self.Eb[i] = Bn, Eb

    def check(self, i, p, buf, label=""):
        """Parameter i's fp32 values against the reference within the accumulated bounds; returns the achieved
        fractions of the bounds (param, momentum)."""
        out = []
        for name, got, ref, bound in (("param", p, self.P[i], self.Ep[i]), ("momentum", buf, self.B[i], self.Eb[i])):
            got = got.detach().double().cpu().reshape(ref.shape)
            assert torch.isfinite(got).all(), (label, i, name, "non-finite")
            frac = ((got - ref).abs() / (bound + TINY)).max().item() if ref.numel() else 0.0
            assert frac <= 1.0, (label, i, name, frac)
            out.append(frac)
        return out
