"""The pre-activation ResNet-18/34 on the CPU: structure, the independent functional twin (tests/_preact_ref.py), and
the argument errors of the missing fp32 / SyncBatchNorm paths."""
import pytest
import torch
import torch.nn.functional as F

from tests import _preact_ref as P
from tests._resnet_ref import twin_state


def _model(depth=18, seed=0, **kw):
    from ddpx.models import build_model
    torch.manual_seed(seed)
    return build_model(f"preact_resnet{depth}", device="cpu", **kw)


@pytest.mark.parametrize("depth,params,bn_params", [(18, 11_172_170, 7_808), (34, 21_280_330, 15_232)])
def test_structure(depth, params, bn_params):
    """By hand, depth 18 (34): convolutions 11,159,232 (21,259,968), BatchNorms 2 * 3,904 (2 * 7,616), head 5,130."""
    from ddpx.models import PreActResNet
    from ddpx.ops.plan import conv_adds, conv_blocks, conv_joins
    m = _model(depth)
    assert isinstance(m, PreActResNet) and not m.use_native
    assert sum(p.numel() for p in m.parameters()) == params
    assert sum(p.numel() for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d) for p in b.parameters()) == bn_params
    assert tuple(m.state_dict().keys()) == m.STATE_KEYS
    assert all(c.bias is None for c in m.modules() if isinstance(c, torch.nn.Conv2d))
    counts, nblk = P.COUNTS[depth], sum(P.COUNTS[depth])
    (blocks, skip), (stride, join), add = conv_blocks(m), conv_joins(m), conv_adds(m)
    assert len(blocks) == 1 + 2 * nblk and skip == join == [None] * len(blocks)
    first = [1 + 2 * sum(counts[:s]) for s in (1, 2, 3)]  # conv1 of the first block of stages 2-4
    assert [bi for bi, s in enumerate(stride) if s == 2] == first
    # every conv2 (even index >= 2) adds the shortcut that starts two units below; a projection where conv1 strides
    assert [None if a is None else (a[0], a[1] is not None) for a in add] == [None] + [
        v for b in range(nblk) for v in (None, (2 * b, 1 + 2 * b in first))]
    # a unit's BatchNorm is the one that reads its convolution's (summed) output
    assert blocks[0][1] is m.layer1[0].bn1 and blocks[1][1] is m.layer1[0].bn2 and blocks[-1][1] is m.bn
    # grad-ready order of the native backward (per unit, last first: bn, sc_conv, conv) = reverse registration
    ready = [m.classifier.weight, m.classifier.bias]
    for (conv, bn, _), a in zip(blocks[::-1], add[::-1]):
        ready += [bn.weight, bn.bias] + ([a[1].weight] if a is not None and a[1] is not None else []) + [conv.weight]
    want = [p for mod in reversed([mod for mod in m.modules() if list(mod.parameters(recurse=False))])
            for p in mod.parameters(recurse=False)]
    assert len(ready) == len(want) and all(a is b for a, b in zip(ready, want))


@pytest.mark.parametrize("depth,training", [(18, True), (18, False), (34, True)])
def test_model_equals_independent_twin(depth, training):
    """tests/test_resnet18_cpu.py's tolerances."""
    m = _model(depth, seed=3)
    for bn in (mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)):
        for v, lo, hi in ((bn.weight, 0.5, 1.5), (bn.bias, -0.3, 0.3), (bn.running_mean, -0.2, 0.2),
                          (bn.running_var, 0.5, 2.0)):
            v.data.uniform_(lo, hi)
    m.train(training)
    sd = twin_state(m)
    x, t = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    out, ref = m(x), P.twin_forward(sd, x, training, depth)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5), float((out - ref).abs().max())
    F.cross_entropy(out, t).backward()
    F.cross_entropy(ref, t).backward()
    for k, p in m.named_parameters():
        scale = float(p.grad.abs().max()) + 1e-12
        assert float((p.grad - sd[k].grad).abs().max()) <= 1e-4 * scale + 1e-7, k
    for k, v in m.state_dict().items():
        if "running" in k:
            assert torch.allclose(v, sd[k], rtol=1e-5, atol=1e-6), k


def test_argument_errors(capsys):
    from ddpx.models import build_model
    from ddpx.train.app import build_parser
    with pytest.raises(ValueError, match="fp32 add\\+statistics kernel"):
        build_model("preact_resnet18", dtype="fp32", kernels="native", device="cpu")
    with pytest.raises(SystemExit):
        build_parser("t").parse_args(["1", "1", "--model", "preact_resnet34", "--kernels", "native", "--dtype", "fp32"])
    assert "fp32 add+statistics kernel is missing" in capsys.readouterr().err
    build_parser("t").parse_args(["1", "1", "--model", "preact_resnet18", "--kernels", "native", "--dtype", "bf16"])
    m = _model()
    m.sync_bn_comm = object()  # torch-op path: SyncBatchNorm is converted elsewhere, nothing to refuse
    m.use_native = True
    with pytest.raises(ValueError, match="no cross-rank merge"):
        m.sync_bn_comm = object()
