"""References for the basic-block join (plain helper module, no fixtures): float64 forward / backward of
``relu(a*y + b + s)`` on ``tests/_exact.py``'s grid, and ResNet-18 as a functional composition from a ``state_dict``
alone (``tests/test_resnet18_cpu.py`` checks the model against it)."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import _exact as X

JOIN_SHAPES = X.BN_SHAPES + ((5, 9, 9, 64),)  # the last: 405 pixels = 4 pass-1 blocks of 128, the last one ragged


@functools.lru_cache(maxsize=None)
def join_case(shape, proj, seed=0):
    """``X.bn_case`` (y, a, b, mean, rstd, g) plus the second operand and g2.  Identity: res integers in [-8, 8].
    Projection: y2 integers in [-8, 8] with a2 / b2 / mean2 / rstd2 from bn_case's grids.  Everything is a multiple
    of 0.25 of small magnitude, so z = a*y + b + s is exact in fp32.  Channel 0 is forced to contain z == 0 (first
    pixel: y = 0, b = 0, s = 0 with b2 = 0) and the random signs give z < 0 and z > 0 everywhere else."""
    c = dict(X.bn_case(shape, False, seed))
    s = seed * 1000 + hash((shape, proj)) % 997
    C = shape[-1]
    c["g2"] = X.ints(shape, -3, 3, s + 12)
    c["y"], c["b"] = c["y"].clone(), c["b"].clone()
    c["y"][0, 0, 0, 0], c["b"][0] = 0.0, 0.0
    so = X.ints(shape, -8, 8, s + 11)
    so[0, 0, 0, 0] = 0.0
    if proj:
        c["y2"] = so
        c["a2"] = X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (C,), s + 13)
        c["b2"] = X.ints((C,), -8, 8, s + 14) * 0.25
        c["b2"][0] = 0.0
        c["mean2"] = X.ints((C,), -8, 8, s + 15) * 0.25
        c["rstd2"] = X.choice([0.5, 1.0, 2.0], (C,), s + 16)
    else:
        c["res"] = so
    return c


def join_z(c):
    s = c["a2"] * c["y2"] + c["b2"] if "y2" in c else c["res"]
    return c["a"] * c["y"] + c["b"] + s


def join_backward_ref(c, with_g2):
    """dict of the float64 results: m, dbeta, dgamma, dy, terms (and dgamma2, dy2, terms2 in projection mode), terms
    = |a| * (|m| + |c1| + |xhat*c2|) as ``X.bn_backward_ref``."""
    m = torch.where(join_z(c) > 0, c["g"] + (c["g2"] if with_g2 else 0), torch.zeros_like(c["g"]))
    M = m[..., 0].numel()
    r = {"m": m, "dbeta": m.sum((0, 1, 2))}

    def branch(y, a, mean, rstd, sfx):
        xhat = (y - mean) * rstd
        X_ok = (m.abs() * xhat.abs()).sum((0, 1, 2)).max() * 8 < X.EXACT_LIMIT  # multiples of 1/8: exact in fp32
        assert X_ok and m.abs().sum((0, 1, 2)).max() < X.EXACT_LIMIT
        dgamma = (m * xhat).sum((0, 1, 2))
        c1, c2 = r["dbeta"] / M, dgamma / M
        r["dgamma" + sfx] = dgamma
        r["dy" + sfx] = a * (m - c1 - xhat * c2)
        r["terms" + sfx] = a.abs() * (m.abs() + c1.abs() + (xhat * c2).abs())

    branch(c["y"], c["a"], c["mean"], c["rstd"], "")
    if "y2" in c:
        branch(c["y2"], c["a2"], c["mean2"], c["rstd2"], "2")
    return r


# ------------------------------------------------------------------ the independent twin of ResNet-18
def twin_forward(sd, x, training, eps=1e-5, momentum=0.1):
    """CIFAR ResNet-18 logits from a state_dict ``sd`` (running statistics updated in place when ``training``) and
    NCHW input x."""
    def bn(name, x):
        return F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"],
                            sd[f"{name}.bias"], training, momentum, eps)

    x = F.relu(bn("stem.bn", F.conv2d(x, sd["stem.conv.weight"], None, padding=1)))
    for stage in (1, 2, 3, 4):
        for i in (0, 1):
            p = f"layer{stage}.{i}"
            stride = 2 if (stage > 1 and i == 0) else 1
            out = F.relu(bn(f"{p}.bn1", F.conv2d(x, sd[f"{p}.conv1.weight"], None, stride, 1)))
            out = bn(f"{p}.bn2", F.conv2d(out, sd[f"{p}.conv2.weight"], None, 1, 1))
            if stride == 2:
                x = bn(f"{p}.sc_bn", F.conv2d(x, sd[f"{p}.sc_conv.weight"], None, 2, 0))
            x = F.relu(out + x)
    return F.linear(x.mean([2, 3]), sd["classifier.weight"], sd["classifier.bias"])
