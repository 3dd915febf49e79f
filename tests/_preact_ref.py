"""References for the pre-activation residual networks (plain helper module, no fixtures): the
BatchNorm backward with a gradient added on its output side (float64, ``tests/_exact.py``'s grid), and the network as
a functional composition from a ``state_dict`` alone (``tests/test_preact_cpu.py`` checks the model against it)."""
import torch.nn.functional as F

from tests import _exact as X

COUNTS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def bn_backward_add_ref(c, gadd):
    """(dy, dgamma, dbeta, terms) of ``X.bn_backward_ref`` (no pool) on the case ``c`` with gadd added on the output
    side: dgamma / dbeta unchanged, dy = dx + gadd, and gadd joins the magnitudes that scale dy's rounding bound."""
    dy, dgamma, dbeta, terms = X.bn_backward_ref(c["g"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], False)
    return dy + gadd, dgamma, dbeta, terms + gadd.abs()


def twin_forward(sd, x, training, depth=18, eps=1e-5, momentum=0.1):
    """Pre-activation ResNet logits from a state_dict ``sd`` (running statistics updated in place when ``training``)
    and NCHW input x."""
    def bn_relu(name, x):
        return F.relu(F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"],
                                   sd[f"{name}.bias"], training, momentum, eps))

    z = F.conv2d(x, sd["stem.conv.weight"], None, padding=1)
    for stage, n in enumerate(COUNTS[depth], 1):
        for i in range(n):
            p, down = f"layer{stage}.{i}", stage > 1 and i == 0
            act = bn_relu(f"{p}.bn1", z)
            u = F.conv2d(act, sd[f"{p}.conv1.weight"], None, 2 if down else 1, 1)
            y = F.conv2d(bn_relu(f"{p}.bn2", u), sd[f"{p}.conv2.weight"], None, 1, 1)
            z = y + (F.conv2d(act, sd[f"{p}.sc_conv.weight"], None, 2, 0) if down else z)
    return F.linear(bn_relu("bn", z).mean([2, 3]), sd["classifier.weight"], sd["classifier.bias"])
