"""ResNet-18 on the CPU: structure, the independent functional twin (tests/_join_ref.py), and the argument errors of
the missing fp32 / SyncBatchNorm join kernels."""
import pytest
import torch
import torch.nn.functional as F

from tests import _join_ref as J
from tests._resnet_ref import twin_state


def _model(seed=0, **kw):
    from ddpx.models import build_model
    torch.manual_seed(seed)
    return build_model("resnet18", device="cpu", **kw)


def test_structure():
    from ddpx.models import ResNet18
    from ddpx.ops.plan import conv_blocks, conv_joins
    m = _model()
    assert isinstance(m, ResNet18) and not m.use_native
    assert sum(p.numel() for p in m.parameters()) == 11_173_962
    assert tuple(m.state_dict().keys()) == ResNet18.STATE_KEYS
    assert all(c.bias is None for c in m.modules() if isinstance(c, torch.nn.Conv2d))
    # the native graph's description: stem + two entries per basic block; three projections, at stride 2
    blocks, skip = conv_blocks(m)
    stride, join = conv_joins(m)
    assert len(blocks) == 17 and skip == [None] * 17
    assert [bi for bi, s in enumerate(stride) if s == 2] == [5, 9, 13]
    assert [None if j is None else (j[0], j[1] is not None) for j in join] == [None] + [
        None, (0, False), None, (2, False), None, (4, True), None, (6, False), None, (8, True), None, (10, False),
        None, (12, True), None, (14, False)]
    # grad-ready order of the native backward (sc_bn, bn2, sc_conv, conv2, bn1, conv1 per block) = reverse registration
    ready = [m.classifier.weight, m.classifier.bias]
    for bi in range(16, -1, -1):
        (conv, bn, _), j = blocks[bi], join[bi]
        if j is not None and j[1] is not None:
            ready += [j[2].weight, j[2].bias, bn.weight, bn.bias, j[1].weight, conv.weight]
        else:
            ready += [bn.weight, bn.bias, conv.weight]
    want = [p for mod in reversed([mod for mod in m.modules() if list(mod.parameters(recurse=False))])
            for p in mod.parameters(recurse=False)]
    assert len(ready) == len(want) and all(a is b for a, b in zip(ready, want))


@pytest.mark.parametrize("training", [True, False])
def test_model_equals_independent_twin(training):
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
    out, ref = m(x), J.twin_forward(sd, x, training)
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
        build_model("resnet18", dtype="fp32", kernels="native", device="cpu")
    with pytest.raises(SystemExit):
        build_parser("t").parse_args(["1", "1", "--model", "resnet18", "--kernels", "native", "--dtype", "fp32"])
    assert "fp32 join kernels are missing" in capsys.readouterr().err
    build_parser("t").parse_args(["1", "1", "--model", "resnet18", "--kernels", "native", "--dtype", "bf16"])
    m = _model()
    m.sync_bn_comm = object()  # torch-op path: SyncBatchNorm is converted elsewhere, nothing to refuse
    m.use_native = True
    with pytest.raises(ValueError, match="all-reduce between their passes"):
        m.sync_bn_comm = object()
