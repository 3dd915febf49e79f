"""ResNet-20/32/44/56 on the CPU: structure, the independent functional twin (tests/_pad_ref.py, the shortcut written
with F.pad), and the argument errors of the missing fp32 / SyncBatchNorm join kernels."""
import pytest
import torch
import torch.nn.functional as F

from tests import _pad_ref as R
from tests._resnet_ref import twin_state


def _model(name="resnet20", seed=0, **kw):
    from ddpx.models import build_model
    torch.manual_seed(seed)
    return build_model(name, device="cpu", **kw)


def test_structure():
    from ddpx.models import ResNetCifar
    from ddpx.ops.plan import PAD, conv_blocks, conv_joins
    m = _model()
    assert isinstance(m, ResNetCifar) and not m.use_native
    assert sum(p.numel() for p in m.parameters()) == 269_722
    assert tuple(m.state_dict().keys()) == ResNetCifar.STATE_KEYS == m.STATE_KEYS
    m56 = _model("resnet56")
    assert tuple(m56.state_dict().keys()) == m56.STATE_KEYS and len(conv_blocks(m56)[0]) == 55
    convs = [c for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    assert all(c.bias is None for c in convs) and [c.out_channels for c in convs] == [16] * 7 + [32] * 6 + [64] * 6
    # the native graph's description: stem + two entries per basic block; two option-A joins, at stride 2
    blocks, skip = conv_blocks(m)
    stride, join = conv_joins(m)
    assert len(blocks) == 19 and skip == [None] * 19
    assert [bi for bi, s in enumerate(stride) if s == 2] == [7, 13]
    assert join == [None] + [v for k in range(0, 18, 2) for v in (None, (k, PAD if k in (6, 12) else None, None))]
    # grad-ready order of the native backward (bn2, conv2, bn1, conv1 per block) = reverse registration order
    ready = [m.classifier.weight, m.classifier.bias]
    for conv, bn, _ in reversed(blocks):
        ready += [bn.weight, bn.bias, conv.weight]
    want = [p for mod in reversed([mod for mod in m.modules() if list(mod.parameters(recurse=False))])
            for p in mod.parameters(recurse=False)]
    assert len(ready) == len(want) and all(a is b for a, b in zip(ready, want))


@pytest.mark.parametrize("training", [True, False])
def test_model_equals_independent_twin(training):
    """test_resnet18_cpu.py's tolerances."""
    m = _model(seed=3)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.5, 2.0)
    m.train(training)
    sd = twin_state(m)
    x, t = torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    out, ref = m(x), R.twin_forward(sd, x, training, m.n)
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
    with pytest.raises(ValueError, match="fp32 join kernels"):
        build_model("resnet20", dtype="fp32", kernels="native", device="cpu")
    with pytest.raises(SystemExit):
        build_parser("t").parse_args(["1", "1", "--model", "resnet32", "--kernels", "native", "--dtype", "fp32"])
    assert "fp32 join kernels are missing" in capsys.readouterr().err
    for name, depth in (("resnet20", 20), ("resnet32", 32), ("resnet44", 44), ("resnet56", 56)):
        ns = build_parser("t").parse_args(["1", "1", "--model", name, "--kernels", "native", "--dtype", "bf16"])
        assert _model(ns.model).depth == depth
    m = _model()
    m.sync_bn_comm = object()  # torch-op path: SyncBatchNorm is converted elsewhere, nothing to refuse
    m.use_native = True
    with pytest.raises(ValueError, match="all-reduce between their passes"):
        m.sync_bn_comm = object()
