"""Element-exact tests of the basic-block join kernels (csrc/kernels/bn_join.hip): relu(a*y + b + s) with s the
identity operand or a second BatchNorm, and its backward, on the integer / eighths grid of tests/_exact.py where z and
every sum are exact in fp32.  References: tests/_join_ref.py (float64)."""
import pytest
import torch

from tests import _exact as X
from tests import _join_ref as J

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ACT = ("y", "g", "g2", "res", "y2")


def _case(shape, proj, gpu):
    c = J.join_case(shape, proj)
    z = J.join_z(c)
    assert (z == 0).any() and (z < 0).any() and (z > 0).any()  # the strict mask is exercised
    d = {k: v.to(BF16 if k in ACT else F32).to(gpu) for k, v in c.items()}
    ops = dict(proj=tuple(d[k] for k in ("y2", "a2", "b2", "mean2", "rstd2"))) if proj else dict(res=d["res"])
    return c, d, ops


def _backward(K, d, ops, shape, with_g2, **kw):
    return K.bn_join_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], *shape,
                              gout2=d["g2"] if with_g2 else None, **ops, **kw)


@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("shape", J.JOIN_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_bn_join_forward_exact(gpu, shape, proj):
    from ddpx.ops import conv as K
    c, d, ops = _case(shape, proj, gpu)
    fwd = dict(proj=ops["proj"][:3]) if proj else ops
    out = K.bn_join(d["y"], d["a"], d["b"], *shape, **fwd)
    X.assert_equal(out, X.rounded(J.join_z(c).clamp_min(0), BF16), f"bn_join {shape} proj {proj}")


@pytest.mark.parametrize("with_g2", [False, True], ids=["g", "g+g2"])
@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("shape", J.JOIN_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_bn_join_backward_exact(gpu, shape, proj, with_g2):
    """dbeta / dgamma (/ dgamma2) equal the float64 sums in the stored fp32, stored bf16 and accumulated modes; gm
    equals bf16(m); dy (/ dy2) per element within one bf16 ulp of the largest term of a*(m - c1 - xhat*c2), the bound
    test_bn_backward_exact derives: 2^-8 * |a| * (|m| + |c1| + |xhat*c2|).  Nothing measured."""
    from ddpx.ops import conv as K
    N, H, W, C = shape
    c, d, ops = _case(shape, proj, gpu)
    r = J.join_backward_ref(c, with_g2)
    names = ("dgamma", "dbeta") + (("dgamma2", "dbeta2") if proj else ())
    want = {n: r[n if n != "dbeta2" else "dbeta"] for n in names}
    f32 = {n: torch.full((C,), 7.0, device=gpu) for n in names}
    dy, aux = _backward(K, d, ops, shape, with_g2, **f32)
    acc = {n: v.clone() for n, v in f32.items()}
    _backward(K, d, ops, shape, with_g2, accumulate=True, accumulate2=proj, **acc)
    b16 = {n: torch.full((C,), 7.0, dtype=BF16, device=gpu) for n in names}
    _backward(K, d, ops, shape, with_g2, **b16)
    what = f"bn_join_backward {shape} proj {proj} g2 {with_g2}"
    for n in names:
        X.assert_equal(f32[n], X.rounded(want[n], F32), f"{what} {n}")
        X.assert_equal(acc[n], X.rounded(want[n], F32) * 2, f"{what} {n} accumulated")
        X.assert_equal(b16[n], X.rounded(want[n], BF16), f"{what} {n} bf16")
    if not proj:
        X.assert_equal(aux, X.rounded(r["m"].reshape(-1, C), BF16), what + " gm")
    for got, sfx in ((dy, ""), (aux, "2"))[:2 if proj else 1]:
        err = (got.double().cpu().reshape(N, H, W, C) - r["dy" + sfx]).abs()
        bad = ~(err <= r["terms" + sfx] * 2.0 ** -8)
        assert not bad.any(), f"{what} dy{sfx}: {int(bad.sum())} elements past one bf16 ulp of the largest term"


@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
def test_bn_join_backward_reproducible(gpu, proj):
    """Fixed summation order: both passes twice on non-grid operands (fp32 sums that do round) give identical bits."""
    from ddpx.ops import conv as K
    shape = J.JOIN_SHAPES[-1]
    _, d, ops = _case(shape, proj, gpu)
    torch.manual_seed(0)
    for k in ("y", "g", "g2"):
        d[k] = torch.randn_like(d[k], dtype=F32).to(BF16)
    runs = []
    for _ in range(2):
        dg, db = torch.empty(shape[-1], device=gpu), torch.empty(shape[-1], device=gpu)
        runs.append((*_backward(K, d, ops, shape, True, dgamma=dg, dbeta=db), dg, db))
    for u, v in zip(*runs):
        assert torch.equal(X._bits(u), X._bits(v))
