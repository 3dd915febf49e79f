"""References for the scaled global max-pool tail, Cutout and flip test-time augmentation (plain helper module, no
fixtures).

* :func:`gmaxpool_ref` / :func:`gmaxpool_bwd_ref`: the hand-written reference of ``ddpx_gmaxpool`` and its backward on
  ``x [N][S][C]``: ``m = x.amax``, the first index of the maximum through ``(x == m).cumsum(...) == 1``, the scale in
  fp32, one rounding to the storage type (``tests/test_gmaxpool_cpu.py`` checks it against ``F.max_pool2d``);
* :func:`tail_twin_forward`: ResNet-9 with either tail as a functional composition from a ``state_dict`` alone;
* :func:`cutout_params_scalar`: the Cutout draw in plain Python integers.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import _resnet_ref as R

SHAPES = ((3, 16, 8), (2, 16, 72), (5, 1, 8), (2, 5, 16), (4, 16, 512))  # (N, S, C); the last is the model's own
SCALES = (1.0, 0.125, 0.3)


def bits(t):
    """The tensor's bit patterns as integers (bitwise comparisons that tell +0 from -0)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def gmaxpool_ref(x, scale):
    """out [N][C] = round(scale * max_s x[n][s][c]): the maximum exact in x's type, the product in fp32."""
    m = x.amax(1)
    return (m.float() * torch.tensor(scale, dtype=torch.float32)).to(x.dtype)


def gmaxpool_bwd_ref(g, x, scale):
    """gx [N][S][C]: round(scale * g[n][c]) at the lowest s with x[n][s][c] equal to the maximum, +0 elsewhere."""
    m = x.amax(1, keepdim=True)
    eq = x == m
    first = eq & (eq.cumsum(1) == 1)
    val = (g.float() * torch.tensor(scale, dtype=torch.float32)).to(x.dtype)
    return torch.where(first, val[:, None, :].expand_as(x), torch.zeros((), dtype=x.dtype))


def random_case(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    N, S, C = shape
    return torch.randn(N, S, C, generator=gen).to(dtype), torch.randn(N, C, generator=gen).to(dtype)


def tied_case(shape, dtype, seed):
    """Values from {0, 1, 2}: with S = 16 most columns hold several maxima."""
    gen = torch.Generator().manual_seed(seed)
    N, S, C = shape
    x = torch.randint(0, 3, (N, S, C), generator=gen).to(dtype)
    g = (torch.randint(1, 9, (N, C), generator=gen) * 0.25).to(dtype)  # non-zero: the routed entry is visible
    return x, g


def tail_twin_forward(sd, x, training, tail="avg", tail_scale=1.0, eps=1e-5, momentum=0.1):
    """``tests/_resnet_ref.py::twin_forward`` with the tail chosen: logits from a state_dict and NCHW input."""
    if tail == "avg":
        return R.twin_forward(sd, x, training, eps, momentum)

    def block(name, x, pool):
        x = F.conv2d(x, sd[f"{name}.conv.weight"], None, padding=1)
        x = F.batch_norm(x, sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"], sd[f"{name}.bn.weight"],
                         sd[f"{name}.bn.bias"], training, momentum, eps)
        x = F.relu(x)
        return F.max_pool2d(x, 2) if pool else x

    x = block("layer1", block("prep", x, False), True)
    x = x + block("res1.1", block("res1.0", x, False), False)
    x = block("layer3", block("layer2", x, True), True)
    x = x + block("res3.1", block("res3.0", x, False), False)
    feat = x.amax((2, 3)) * tail_scale
    return F.linear(feat, sd["classifier.weight"], sd["classifier.bias"])


# ------------------------------------------------------------------ Cutout: the draw in Python integers
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def cutout_params_scalar(seed, batch, H, W, salt):
    """[(cy, cx)] of samples 0 .. batch - 1: rc = splitmix64(r ^ salt), r the sample's crop / flip hash."""
    out = []
    for b in range(batch):
        r = _splitmix64((seed & _M64) ^ ((0xD1B54A32D192ED03 * (b + 1)) & _M64))
        rc = _splitmix64(r ^ salt)
        out.append((rc % H, (rc >> 20) % W))
    return out


def cutout_box(cy, cx, S, H, W):
    """(y0, y1, x0, x1): rows [cy - S // 2, cy - S // 2 + S) and the same columns, clipped to the image."""
    y0, x0 = cy - S // 2, cx - S // 2
    return max(y0, 0), min(y0 + S, H), max(x0, 0), min(x0 + S, W)
