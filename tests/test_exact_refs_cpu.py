"""The element-exact helper (tests/_exact.py) checked against torch on the CPU: its float64 references must be
``F.conv2d`` / autograd themselves, and the magnitude condition must hold for every shape the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

_GEOMS = X.CONV_GEOMS
_SMALL_CH = ((3, 16), (8, 8), (16, 24))


@pytest.mark.parametrize("geom", _GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_conv_refs_equal_torch_float64(geom):
    """Forward, data gradient and weight gradient, non-square geometries included: integer operands, so the
    float64 results are exact and must be equal, not close."""
    for chans in _SMALL_CH:
        c = X.conv_case(geom, chans)
        x = c["x"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        y = F.conv2d(x, w, padding=1)
        y.backward(c["dy"].permute(0, 3, 1, 2).contiguous())
        assert torch.equal(c["y"], y.detach().permute(0, 2, 3, 1))
        assert torch.equal(c["dx"], x.grad.permute(0, 2, 3, 1))
        assert torch.equal(c["dw"], w.grad)
        dyn = c["dy"].permute(0, 3, 1, 2).contiguous()
        assert torch.equal(c["dx"], torch.nn.grad.conv2d_input(x.shape, c["w"], dyn, padding=1).permute(0, 2, 3, 1))
        assert torch.equal(c["dw"], torch.nn.grad.conv2d_weight(x.detach(), w.shape, dyn, padding=1))


def test_conv_case_is_cached_and_integer():
    c = X.conv_case((3, 7, 7), (64, 64))
    assert X.conv_case((3, 7, 7), (64, 64)) is c
    for k in ("x", "w", "dy", "bias", "y", "dx", "dw"):
        assert torch.equal(c[k], c[k].round())
    assert c["x"].abs().max() <= X.CONV_XMAX and c["w"].abs().max() <= X.CONV_WMAX


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_routing_ref_equals_autograd_on_ties(shape, pool):
    """relu(a*y + b) [+ 2x2 max-pool] and its routed gradient against torch CPU autograd in float64, on inputs full
    of ties (small integers; negative scales)."""
    c = X.bn_case(shape, pool)
    y, a, b, g = c["y"], c["a"], c["b"], c["g"]
    if pool:  # the point of the inputs: ties for the maximum inside windows do occur
        r = X._windows((a * y + b).clamp_min(0))
        assert ((r == r.max(-1, keepdim=True).values).sum(-1) > 1).float().mean() > 0.1
    z = (a * y + b).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = F.relu(z)
    if pool:
        out = F.max_pool2d(out, 2)
    out.backward(g.permute(0, 3, 1, 2).contiguous())
    assert torch.equal(X.bn_apply_ref(y, a, b, pool), out.detach().permute(0, 2, 3, 1))
    assert torch.equal(X.route_ref(g, y, a, b, pool), z.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("pool", [False, True])
def test_bn_backward_ref_equals_autograd(pool):
    """dy, dgamma, dbeta of BatchNorm (given mean / rstd as constants of the affine map) + ReLU + pool."""
    shape = X.BN_SHAPES[1]
    c = X.bn_case(shape, pool)
    y, a, b, mean, rstd, g = (c[k] for k in ("y", "a", "b", "mean", "rstd", "g"))
    b = b + 0.1  # keeps z = a*y + b away from 0, where torch's differently rounded z could flip the ReLU mask
    dy, dgamma, dbeta, terms = X.bn_backward_ref(g, y, a, b, mean, rstd, pool)
    # autograd through batch statistics: use the batch's own mean / rstd so that torch's formula applies
    M = y.shape[0] * y.shape[1] * y.shape[2]
    mu = y.mean((0, 1, 2))
    rs = 1.0 / (y.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()
    gamma = a / rs
    beta = b + mu * a
    yr = y.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    xh = (yr - yr.mean((0, 1, 2))) / (yr.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()
    out = F.relu(xh * gr + br).permute(0, 3, 1, 2)
    if pool:
        out = F.max_pool2d(out, 2)
    out.backward(g.permute(0, 3, 1, 2).contiguous())
    dy2, dgamma2, dbeta2, _ = X.bn_backward_ref(g, y, a, b, mu, rs, pool)
    assert torch.allclose(dy2, yr.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(dgamma2, gr.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(dbeta2, br.grad, rtol=1e-9, atol=1e-9)
    assert dy.shape == y.shape and terms.shape == y.shape and M == y[..., 0].numel()
    assert torch.equal(dbeta, X.route_ref(g, y, a, b, pool).sum((0, 1, 2)))


def test_magnitude_condition_holds_for_every_shape():
    for K in X.GEMM_KS:
        X.require_exact(X.GEMM_AMAX, X.GEMM_BMAX, K, "gemm")
    pairs = X.conv_pairs() + [(g, c) for g in X.CONV_CFG_GEOMS for c in X.CONV_CHANNELS + X.WGRAD_CHANNELS]
    for (N, H, W), (Ci, Co) in pairs:
        X.require_exact(X.CONV_XMAX, X.CONV_WMAX, 9 * X.padded_channels(Ci), "conv fwd")
        X.require_exact(X.CONV_XMAX, X.CONV_WMAX, 9 * Co, "conv dgrad")
        X.require_exact(X.CONV_XMAX, X.CONV_XMAX, N * H * W, "conv wgrad")
    with pytest.raises(AssertionError):
        X.require_exact(4, 4, 2 ** 20)


def test_conv_pairs_cover_the_lists():
    pairs = X.conv_pairs()
    for g in X.CONV_GEOMS:
        assert sum(1 for p in pairs if p[0] == g) >= 2
    for c in X.CONV_CHANNELS:
        gs = [p[0] for p in pairs if p[1] == c]
        assert len(gs) >= 3
    assert any(64 % g[2] == 0 and c[0] % 64 == 0 for g, c in pairs)
    assert any(64 % g[2] != 0 and c[0] % 64 == 0 for g, c in pairs)
    assert any(c[0] % 64 != 0 for g, c in pairs)


def test_helpers_guard_poison_and_compare():
    buf, view = X.guarded(5, 8, torch.float32, "cpu")
    view.zero_()
    X.assert_guard(buf, 5, 8, "ok")
    buf[0, 3] = 1.0
    with pytest.raises(AssertionError, match="guard"):
        X.assert_guard(buf, 5, 8, "spill")
    p = X.poisoned(torch.ones(4, 8), "cpu")
    assert p.stride(0) == 16 and torch.isnan(p._base[:, 8:]).all() and not torch.isnan(p).any()
    X.assert_equal(torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0]), "signed zero")
    with pytest.raises(AssertionError, match="1 of 2"):
        X.assert_equal(torch.tensor([float("nan"), 1.0]), torch.tensor([float("nan"), 1.0]), "nan")
    m, pos = X.mask_operand((64, 16), 1)
    assert torch.equal(pos, (m.double() > 0).double())
    assert torch.equal(X.rounded(torch.tensor([257.0], dtype=torch.float64), torch.bfloat16),
                       torch.tensor([256.0], dtype=torch.bfloat16))
