"""The scaled global max-pool tail on the CPU: the hand-written reference of ``tests/_tail_ref.py`` against
``F.max_pool2d`` (forward and autograd, tie-free and tied inputs), ResNet-9 with ``tail="max"`` against a functional
twin, the unchanged default model, and the argument errors."""
import pytest
import torch
import torch.nn.functional as F

from tests import _resnet_ref as R
from tests import _tail_ref as T


def _torch_pool(x, g, scale, hw):
    """F.max_pool2d over the whole (H, W) window of x [N][S][C] seen as NCHW, times scale, and its autograd gradient
    for the output gradient g [N][C]; both back in [N][S][C] / [N][C] order."""
    N, S, C = x.shape
    H, W = hw
    xn = x.reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = F.max_pool2d(xn, (H, W)).flatten(1) * scale
    out.backward(g)
    return out.detach(), xn.grad.permute(0, 2, 3, 1).reshape(N, S, C)


@pytest.mark.parametrize("case", ["random", "tied"])
@pytest.mark.parametrize("shape,hw", [((3, 16, 8), (4, 4)), ((2, 5, 16), (1, 5)), ((5, 1, 8), (1, 1)),
                                      ((2, 12, 8), (3, 4))], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("scale", T.SCALES)
def test_reference_equals_max_pool2d(case, shape, hw, scale):
    x, g = (T.random_case if case == "random" else T.tied_case)(shape, torch.float32, seed=3)
    out, gx = _torch_pool(x, g, scale, hw)
    assert torch.equal(T.gmaxpool_ref(x, scale), out)
    ref = T.gmaxpool_bwd_ref(g, x, scale)
    assert torch.equal(ref, gx)
    assert int((ref != 0).sum()) == shape[0] * shape[2]  # exactly one routed entry per (n, c) column
    if case == "tied" and shape[1] > 4:
        m = x.amax(1, keepdim=True)
        assert ((x == m).sum(1) > 1).float().mean() > 0.5  # most columns do hold several maxima


def test_reference_rounds_once_in_bf16():
    x, g = T.random_case((3, 16, 8), torch.bfloat16, seed=1)
    out = T.gmaxpool_ref(x, 0.3)
    assert out.dtype == torch.bfloat16
    exact = x.double().amax(1) * float(torch.tensor(0.3, dtype=torch.float32))
    assert ((out.double() - exact).abs() <= exact.abs() * 2.0 ** -8 + 1e-30).all()  # half a bf16 ulp
    assert torch.equal(T.gmaxpool_ref(x, 0.125).double(), x.double().amax(1) * 0.125)  # a power of two: exact


def test_nan_stays_in_the_reference():
    x, _ = T.random_case((2, 5, 16), torch.float32, seed=2)
    x[1, 3, 7] = float("nan")
    out = T.gmaxpool_ref(x, 0.125)
    assert torch.isnan(out[1, 7]) and int(torch.isnan(out).sum()) == 1


def _model(seed=0, **kw):
    from ddpx.models import build_model
    torch.manual_seed(seed)
    return build_model("resnet9", device="cpu", **kw)


@pytest.mark.parametrize("training", [True, False])
def test_max_tail_model_equals_functional_twin(training):
    m = _model(seed=3, tail="max", tail_scale=0.125)
    assert (m.tail, m.tail_scale) == ("max", 0.125)
    m.train(training)
    sd = R.twin_state(m)
    x = torch.randn(6, 3, 32, 32)
    t = torch.randint(0, 10, (6,))
    out = m(x)
    ref = T.tail_twin_forward(sd, x, training, "max", 0.125)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5), float((out - ref).abs().max())
    assert not torch.allclose(out, R.twin_forward(R.twin_state(m), x, False), rtol=1e-3, atol=1e-3)  # not the avg tail
    F.cross_entropy(out, t).backward()
    F.cross_entropy(ref, t).backward()
    for k, p in m.named_parameters():
        scale = float(p.grad.abs().max()) + 1e-12
        assert float((p.grad - sd[k].grad).abs().max()) <= 1e-4 * scale + 1e-7, k
    loss, logits = m.forward_loss(x, t)
    assert logits is not None and torch.isfinite(loss)


def test_default_model_is_unchanged():
    from ddpx.models import ResNet9
    a, b = _model(seed=5), _model(seed=5, tail="avg", tail_scale=1.0)
    torch.manual_seed(5)
    c = ResNet9()
    assert (a.tail, a.tail_scale) == ("avg", 1.0)
    assert tuple(a.state_dict().keys()) == tuple(c.state_dict().keys()) == ResNet9.STATE_KEYS
    assert tuple(_model(tail="max", tail_scale=0.125).state_dict().keys()) == ResNet9.STATE_KEYS
    x = torch.randn(4, 3, 32, 32)
    a.eval(), b.eval(), c.eval()
    with torch.no_grad():
        want = R.twin_forward(R.twin_state(a), x, False)
        assert torch.equal(a(x), b(x)) and torch.equal(a(x), c(x))
        assert torch.allclose(a(x), want, rtol=1e-5, atol=1e-5)


def test_argument_errors():
    from ddpx.models import ResNet9, build_model
    with pytest.raises(ValueError):
        ResNet9(tail="avg", tail_scale=0.125)
    with pytest.raises(ValueError):
        ResNet9(tail="min")
    with pytest.raises(ValueError):
        ResNet9(tail="max", tail_scale=float("nan"))
    with pytest.raises(ValueError):
        build_model("vgg", device="cpu", tail="max")
    with pytest.raises(ValueError):
        build_model("mlp", device="cpu", hidden=64, tail_scale=0.125)
    assert build_model("vgg", device="cpu", tail="avg", tail_scale=1.0) is not None
