"""References for the residual additions (plain helper module, no fixtures).

* float64 references of the two BatchNorm-kernel additions, built from ``tests/_exact.py``'s: the apply pass with a
  skip operand, and the backward with a second gradient (the one-gradient references applied to g1 + g2);
* the exact-grid inputs for them: ``res`` integers in [-8, 8], ``g2`` integers in [-3, 3];
* :func:`twin_forward`: ResNet-9 as a functional composition from a ``state_dict`` alone (no model code) — the
  arbiter of the torch references the GPU tests compare against (``tests/test_resnet_cpu.py`` checks the model
  against it).
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import _exact as X


def apply_res_ref(y, a, b, res, relu=True):
    """res + relu(a*y + b); y, res [N,H,W,C] float64 (no pool: a skip connection joins at equal resolution)."""
    return res + X.bn_apply_ref(y, a, b, False, relu)


def route_ref_2g(g1, g2, y, a, b, pool):
    return X.route_ref(g1 + g2, y, a, b, pool)


def bn_backward_ref_2g(g1, g2, y, a, b, mean, rstd, pool):
    """(dy, dgamma, dbeta, terms) of the block below a residual block: its output's gradient is g1 + g2."""
    return X.bn_backward_ref(g1 + g2, y, a, b, mean, rstd, pool)


@functools.lru_cache(maxsize=None)
def res_case(shape, pool, seed=0):
    """``X.bn_case`` plus res (integers in [-8, 8], full resolution) and g2 (integers in [-3, 3], g's shape) from
    other seeds.  res + relu(a*y + b) is at most 8 + (2*8 + 2) = 26, a multiple of 0.25: exact in bf16."""
    c = dict(X.bn_case(shape, pool, seed))
    s = seed * 1000 + hash((shape, pool)) % 997
    c["res"] = X.ints(shape, -8, 8, s + 11)
    c["g2"] = X.ints(tuple(c["g"].shape), -3, 3, s + 12)
    return c


@functools.lru_cache(maxsize=None)
def unrounded_case(shape, pool, seed=0):
    """g1 from {-64, 64}, g2 from {-0.25, 0.25}: g1 + g2 = +-64.25 / +-63.75 needs 9 significant bits, so a bf16
    round of the sum gives +-64 and the exact dbeta / dgamma tell the two apart."""
    c = dict(X.bn_case(shape, pool, seed))
    s = seed * 1000 + hash((shape, pool)) % 997
    c["g"] = X.choice([-64.0, 64.0], tuple(c["g"].shape), s + 21)
    c["g2"] = X.choice([-0.25, 0.25], tuple(c["g"].shape), s + 22)
    return c


def require_exact_sums(gz, xhat, g_unit=1, x_unit=8):
    """The magnitude conditions of the exact dbeta / dgamma: gz is a multiple of 1/g_unit and xhat of 1/x_unit, and
    the sums of magnitudes, counted in those units, stay below 2**24 — so fp32 holds every partial sum in any
    order.  With the defaults: sum |gz| |xhat| * 8 < 2**24 and sum |gz| < 2**24."""
    assert torch.equal(gz * g_unit, (gz * g_unit).round()) and torch.equal(xhat * x_unit, (xhat * x_unit).round())
    assert (gz.abs() * xhat.abs()).sum((0, 1, 2)).max() * g_unit * x_unit < X.EXACT_LIMIT
    assert gz.abs().sum((0, 1, 2)).max() * g_unit < X.EXACT_LIMIT


# ------------------------------------------------------------------ the independent twin
BLOCKS = (("prep", False), ("layer1", True), ("res1.0", False), ("res1.1", False), ("layer2", True),
          ("layer3", True), ("res3.0", False), ("res3.1", False))


def twin_forward(sd, x, training, eps=1e-5, momentum=0.1):
    """ResNet-9 logits from a state_dict ``sd`` (tensors; the running statistics are updated in place when
    ``training``, as the modules do) and NCHW input x."""
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
    return F.linear(x.mean([2, 3]), sd["classifier.weight"], sd["classifier.bias"])


def twin_state(model, dtype=None, device=None):
    """Detached copies of a model's state_dict (parameters require grad), for :func:`twin_forward`."""
    sd = {}
    params = dict(model.named_parameters())
    for k, v in model.state_dict().items():
        t = v.detach().clone()
        if t.is_floating_point() and dtype is not None:
            t = t.to(dtype)
        if device is not None:
            t = t.to(device)
        if k in params:
            t.requires_grad_(True)
        sd[k] = t
    return sd
