"""Mixup / CutMix for the device-resident loader: configuration, the Beta quantile table and the CPU twin of
the kernel's per-batch draw (``csrc/kernels/data_augment.hip``: ``mix_draw``).

Semantics are timm's "batch" mode: sample b is mixed with sample B - 1 - b of the same batch, and one draw per
batch decides apply / don't apply, Mixup versus CutMix, lam and (CutMix) the box.  The draw is a function of
the batch's augmentation seed alone, from the same counter hash as the crop / flip stream, so it needs no
state: a captured step draws it on the device and ``--resume`` needs nothing new.

lam ~ Beta(alpha, alpha) is taken from a quantile table of 1024 equal-probability bins built here with numpy;
the kernel and the CPU twin index the same table, which is what makes their batches bit-identical.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

BINS = 1024
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2
_SALT = 0x8CB92BA72F3D8DD7
_M64 = (1 << 64) - 1
_P24 = 1 << 24

ROW_DTYPE = np.dtype([("lam", "<f4"), ("cut_h", "<i4"), ("cut_w", "<i4")])


@dataclass(frozen=True)
class MixConfig:
    """``mixup_alpha`` / ``cutmix_alpha``: Beta parameters (0 disables the mode); ``prob``: probability that a
    batch is mixed at all; ``switch_prob``: probability of CutMix when both modes are enabled."""
    mixup_alpha: float = 0.0
    cutmix_alpha: float = 0.0
    prob: float = 1.0
    switch_prob: float = 0.5

    def __post_init__(self):
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0:
            raise ValueError("MixConfig: alphas must be >= 0")
        if not (0.0 <= self.prob <= 1.0 and 0.0 <= self.switch_prob <= 1.0):
            raise ValueError("MixConfig: probabilities must be in [0, 1]")

    @property
    def enabled(self) -> bool:
        return (self.mixup_alpha > 0 or self.cutmix_alpha > 0) and self.prob > 0

    @property
    def modes(self) -> int:
        """Bit 0: Mixup enabled, bit 1: CutMix enabled (the kernel's ``modes`` argument)."""
        return (1 if self.mixup_alpha > 0 else 0) | (2 if self.cutmix_alpha > 0 else 0)

    @property
    def p_apply(self) -> int:
        return int(round(self.prob * _P24))

    @property
    def p_switch(self) -> int:
        return int(round(self.switch_prob * _P24))


def beta_quantiles(alpha: float, bins: int = BINS) -> np.ndarray:
    """Quantiles of Beta(alpha, alpha) at the bin midpoints (i + 1/2) / bins, fp64.

    The lower half comes from integrating the density after the substitution t = u^(1/alpha), which removes
    the t^(alpha - 1) endpoint singularity: F(x) is proportional to the integral over [0, x^alpha] of
    (1 - u^(1/alpha))^(alpha - 1) du, a smooth integrand on [0, 0.5^alpha], normalised by F(1/2) = 1/2.  The
    upper half is the mirror image (the distribution is symmetric), so the table is symmetric by construction."""
    if alpha <= 0:
        raise ValueError("beta_quantiles: alpha must be > 0")
    if bins % 2:
        raise ValueError("beta_quantiles: bins must be even")
    n = 1 << 18
    u = np.linspace(0.0, 0.5 ** alpha, n + 1)
    f = (1.0 - u ** (1.0 / alpha)) ** (alpha - 1.0)
    cum = np.concatenate(([0.0], np.cumsum((f[1:] + f[:-1]) * 0.5)))  # trapezoid; the step cancels below
    cum *= 0.5 / cum[-1]
    p = (np.arange(bins // 2) + 0.5) / bins
    lo = np.interp(p, cum, u) ** (1.0 / alpha)
    return np.concatenate((lo, 1.0 - lo[::-1]))


def build_table(cfg: MixConfig, H: int, W: int) -> np.ndarray:
    """rows[2][BINS] of {lam fp32, cut_h, cut_w int32}: row 0 Mixup (zero box), row 1 CutMix with the box
    extents int(H sqrt(1 - lam)), int(W sqrt(1 - lam)) worked out here in fp64.  A disabled mode's row is
    lam = 1 with a zero box."""
    t = np.zeros((2, BINS), dtype=ROW_DTYPE)
    t["lam"] = 1.0
    if cfg.mixup_alpha > 0:
        t["lam"][0] = np.maximum(beta_quantiles(cfg.mixup_alpha).astype(np.float32), np.float32(1e-30))
    if cfg.cutmix_alpha > 0:
        lam = beta_quantiles(cfg.cutmix_alpha)
        t["lam"][1] = np.maximum(lam.astype(np.float32), np.float32(1e-30))
        r = np.sqrt(1.0 - lam)
        t["cut_h"][1] = (H * r).astype(np.int32)
        t["cut_w"][1] = (W * r).astype(np.int32)
    return t


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


@dataclass(frozen=True)
class MixDraw:
    mode: int = MIX_NONE
    wlam: np.float32 = np.float32(1.0)   # label weight of the sample's own target
    lam: np.float32 = np.float32(1.0)    # Mixup pixel weights lam, oml = 1 - lam (fp32)
    oml: np.float32 = np.float32(0.0)
    box: tuple = (0, 0, 0, 0)            # CutMix: (y0, y1, x0, x1) in output coordinates
    cut: tuple = (0, 0)                  # CutMix: the table's (cut_h, cut_w) the box was clipped from


def batch_draw(seed: int, H: int, W: int, cfg: MixConfig, table: np.ndarray) -> MixDraw:
    """The batch's draw, step for step what the kernel computes (integer hash fields, table lookup, one
    correctly rounded fp32 subtraction / division)."""
    modes = cfg.modes
    r = _splitmix64((seed & _M64) ^ _SALT)
    if not modes or (r & 0xFFFFFF) >= cfg.p_apply:
        return MixDraw()
    cut = ((r >> 24) & 0xFFFFFF) < cfg.p_switch if modes == 3 else modes == 2
    row = table[1 if cut else 0][(r >> 48) & (BINS - 1)]
    if not cut:
        lam = np.float32(row["lam"])
        return MixDraw(MIX_MIXUP, lam, lam, np.float32(1.0) - lam)
    r2 = _splitmix64(r)
    cy, cx = r2 % H, (r2 >> 20) % W
    ch, cw = int(row["cut_h"]), int(row["cut_w"])
    clip = lambda v, hi: min(max(v, 0), hi)  # noqa: E731
    y0, y1 = clip(cy - ch // 2, H), clip(cy + ch // 2, H)
    x0, x1 = clip(cx - cw // 2, W), clip(cx + cw // 2, W)
    wlam = np.float32(1.0) - np.float32((y1 - y0) * (x1 - x0)) / np.float32(H * W)
    return MixDraw(MIX_CUTMIX, np.float32(wlam), np.float32(1.0), np.float32(0.0), (y0, y1, x0, x1),
                   (ch, cw))


class Mixer:
    """A :class:`MixConfig` bound to an image size: the quantile table (host copy for the CPU twin, one device
    copy per device for the kernel) and the per-batch draw."""

    def __init__(self, cfg: MixConfig, H: int, W: int):
        self.cfg, self.H, self.W = cfg, int(H), int(W)
        self.table = build_table(cfg, self.H, self.W)
        self._dev = {}

    def draw(self, seed: int) -> MixDraw:
        return batch_draw(seed, self.H, self.W, self.cfg, self.table)

    def device_table(self, device):
        """The table as the kernel reads it: [2][BINS] rows of 12 bytes, uploaded once per device."""
        t = self._dev.get(device)
        if t is None:
            raw = np.frombuffer(self.table.tobytes(), dtype=np.int32).copy()
            t = self._dev[device] = torch.from_numpy(raw).to(device)
        return t
