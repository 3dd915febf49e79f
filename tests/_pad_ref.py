"""References for the option-A shortcut (plain helper module, no fixtures): the exact-grid case of the pad join (the
identity case of ``tests/_join_ref.py`` whose ``res`` is the materialised padded shortcut), the zero insertion of a
compact skip gradient, and ResNet-20/32/44/56 as a functional composition from a ``state_dict`` alone."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import _exact as X
from tests import _join_ref as J


def out_hw(Hx, Wx):
    return (Hx + 1) // 2, (Wx + 1) // 2


def pad_shortcut(x, C):
    """NHWC x [N, Hx, Wx, C/2] -> [N, H, W, C]: every second pixel, C/4 zero channels on each side."""
    return F.pad(x[:, ::2, ::2, :], (C // 4, C // 4))


def zero_inserted(gs, H, W):
    """Compact gs [N, (H+1)//2, (W+1)//2, C] -> [N, H, W, C] with gs at the even pixels and 0 elsewhere."""
    out = torch.zeros((gs.shape[0], H, W, gs.shape[-1]), dtype=gs.dtype, device=gs.device)
    out[:, ::2, ::2, :] = gs
    return out


@functools.lru_cache(maxsize=None)
def pad_case(N, Hx, Wx, C):
    """``J.join_case`` at the join's shape with x integers in [-8, 8] and res = pad_shortcut(x).  z == 0 is forced
    in a padded channel (0: join_case's) and in an unpadded one (C/4); both regions must show all three signs."""
    c = dict(J.join_case((N, *out_hw(Hx, Wx), C), False))
    c["y"], c["b"] = c["y"].clone(), c["b"].clone()
    x = X.ints((N, Hx, Wx, C // 2), -8, 8, 77 + Hx + C)
    x[0, 0, 0, 0], c["y"][0, 0, 0, C // 4], c["b"][C // 4] = 0.0, 0.0, 0.0
    c["x"], c["res"] = x, pad_shortcut(x, C)
    z = J.join_z(c)
    mid = torch.zeros(C, dtype=torch.bool)
    mid[C // 4:3 * C // 4] = True
    for part in (z[..., mid], z[..., ~mid]):
        assert (part == 0).any() and (part < 0).any() and (part > 0).any()
    return c


def twin_forward(sd, x, training, n, eps=1e-5, momentum=0.1):
    """CIFAR ResNet-(6n+2) logits from a state_dict ``sd`` (running statistics updated in place when ``training``)
    and NCHW input x; the shortcut of a downsampling block is written out with ``F.pad``."""
    def bn(name, x):
        return F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"],
                            sd[f"{name}.bias"], training, momentum, eps)

    x = F.relu(bn("stem.bn", F.conv2d(x, sd["stem.conv.weight"], None, padding=1)))
    for stage in (1, 2, 3):
        for i in range(n):
            p = f"layer{stage}.{i}"
            stride = 2 if (stage > 1 and i == 0) else 1
            out = F.relu(bn(f"{p}.bn1", F.conv2d(x, sd[f"{p}.conv1.weight"], None, stride, 1)))
            out = bn(f"{p}.bn2", F.conv2d(out, sd[f"{p}.conv2.weight"], None, 1, 1))
            if stride == 2:
                C = out.shape[1]
                x = F.pad(x[:, :, ::2, ::2], (0, 0, 0, 0, C // 4, C // 4))
            x = F.relu(out + x)
    return F.linear(x.mean([2, 3]), sd["classifier.weight"], sd["classifier.bias"])
