"""Element-exact tests of the option-A join kernels (csrc/kernels/bn_join.hip, ``pad=`` / ``gout2_sub=``) on the grid
of tests/_exact.py: the reference is tests/_join_ref.py's float64 join on the materialised padded shortcut."""
import pytest
import torch

from tests import _exact as X
from tests import _join_ref as J
from tests import _pad_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ACT = ("y", "g", "g2", "res", "x")
PAD_SHAPES = ((2, 8, 8, 32), (3, 5, 9, 64), (1, 1, 1, 32), (5, 17, 18, 64))  # (N, Hx, Wx, C)
ids = lambda v: "x".join(map(str, v))  # noqa: E731


def _case(xs, gpu):
    N, Hx, Wx, C = xs
    c = R.pad_case(*xs)
    return c, {k: v.to(BF16 if k in ACT else F32).to(gpu) for k, v in c.items()}, (N, *R.out_hw(Hx, Wx), C)


def _backward(K, d, shape, **kw):
    return K.bn_join_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], *shape, **kw)


@pytest.mark.parametrize("xs", PAD_SHAPES, ids=ids)
def test_pad_forward_exact(gpu, xs):
    from ddpx.ops import conv as K
    c, d, shape = _case(xs, gpu)
    out = K.bn_join(d["y"], d["a"], d["b"], *shape, pad=d["x"])
    X.assert_equal(out, X.rounded(J.join_z(c).clamp_min(0), BF16), f"bn_join pad {xs}")
    assert torch.equal(X._bits(out), X._bits(K.bn_join(d["y"], d["a"], d["b"], *shape, res=d["res"])))


@pytest.mark.parametrize("with_g2", [False, True], ids=["g", "g+g2"])
@pytest.mark.parametrize("xs", PAD_SHAPES, ids=ids)
def test_pad_backward_exact(gpu, xs, with_g2):
    """dbeta / dgamma equal the float64 sums in the stored fp32, stored bf16 and accumulated modes; gs equals
    bf16(m)[..., C/4:3C/4]; dy within test_bn_join_backward_exact's bound 2^-8 * |a| * (|m| + |c1| + |xhat*c2|)."""
    from ddpx.ops import conv as K
    c, d, shape = _case(xs, gpu)
    N, H, W, C = shape
    r = J.join_backward_ref(c, with_g2)
    kw = dict(pad=d["x"], gout2=d["g2"] if with_g2 else None)
    f32 = {n: torch.full((C,), 7.0, device=gpu) for n in ("dgamma", "dbeta")}
    dy, gs = _backward(K, d, shape, **kw, **f32)
    acc = {n: v.clone() for n, v in f32.items()}
    _backward(K, d, shape, accumulate=True, **kw, **acc)
    b16 = {n: torch.full((C,), 7.0, dtype=BF16, device=gpu) for n in f32}
    _backward(K, d, shape, **kw, **b16)
    what = f"bn_join_backward pad {xs} g2 {with_g2}"
    for n in f32:
        X.assert_equal(f32[n], X.rounded(r[n], F32), f"{what} {n}")
        X.assert_equal(acc[n], X.rounded(r[n], F32) * 2, f"{what} {n} accumulated")
        X.assert_equal(b16[n], X.rounded(r[n], BF16), f"{what} {n} bf16")
    X.assert_equal(gs, X.rounded(r["m"][..., C // 4:3 * C // 4].contiguous(), BF16), what + " gs")
    err = (dy.double().cpu().reshape(N, H, W, C) - r["dy"]).abs()
    bad = ~(err <= r["terms"] * 2.0 ** -8)
    assert not bad.any(), f"{what} dy: {int(bad.sum())} elements past one bf16 ulp of the largest term"


@pytest.mark.parametrize("mode,shape", [("res", (2, 8, 8, 16)), ("res", (3, 5, 9, 32)), ("pad", PAD_SHAPES[1])],
                         ids=["identity-2x8x8x16", "identity-3x5x9x32", "pad-3x5x9x64"])
def test_strided_second_gradient_equals_dense(gpu, mode, shape):
    """gout2_sub=gs against gout2=zero_inserted(gs): dy, gm (or gs), dgamma and dbeta under torch.equal.  The pad
    case is the downsampling block directly below another (depth 8)."""
    from ddpx.ops import conv as K
    if mode == "pad":
        _, d, shape = _case(shape, gpu)
        so = dict(pad=d["x"])
    else:
        d = {k: v.to(BF16 if k in ACT else F32).to(gpu) for k, v in J.join_case(shape, False).items()}
        so = dict(res=d["res"])
    N, H, W, C = shape
    sub = X.ints((N, *R.out_hw(H, W), C), -3, 3, 5).to(BF16).to(gpu)
    runs = []
    for g2 in (dict(gout2_sub=sub), dict(gout2=R.zero_inserted(sub, H, W))):
        dg, db = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
        runs.append((*_backward(K, d, shape, **so, **g2, dgamma=dg, dbeta=db), dg, db))
    for name, u, v in zip(("dy", "aux", "dgamma", "dbeta"), *runs):
        assert torch.equal(u, v), name


def test_pad_backward_reproducible(gpu):
    """Fixed summation order: twice on non-grid operands (fp32 sums that do round), identical bits."""
    from ddpx.ops import conv as K
    _, d, shape = _case(PAD_SHAPES[-1], gpu)
    torch.manual_seed(0)
    for k in ("y", "g", "g2"):
        d[k] = torch.randn_like(d[k], dtype=F32).to(BF16)
    runs = []
    for _ in range(2):
        dg, db = torch.empty(shape[-1], device=gpu), torch.empty(shape[-1], device=gpu)
        runs.append((*_backward(K, d, shape, pad=d["x"], gout2=d["g2"], dgamma=dg, dbeta=db), dg, db))
    for u, v in zip(*runs):
        assert torch.equal(X._bits(u), X._bits(v))


def test_pad_argument_errors(gpu):
    from ddpx.ops import conv as K
    _, d, shape = _case(PAD_SHAPES[0], gpu)
    N, H, W, C = shape
    with pytest.raises(ValueError, match="C % 32"):
        K.bn_join(d["y"].new_zeros(N, H, W, 48), d["a"].new_zeros(48), d["b"].new_zeros(48), N, H, W, 48,
                  pad=d["x"].new_zeros(N, 8, 8, 24))
    with pytest.raises(ValueError, match="stride-2 block"):
        K.bn_join(d["y"], d["a"], d["b"], *shape, pad=d["x"][:, :6].contiguous())
    sub = d["g2"][:, ::2, ::2].contiguous()
    with pytest.raises(ValueError, match="gout2 and gout2_sub together"):
        _backward(K, d, shape, pad=d["x"], gout2=d["g2"], gout2_sub=sub)
