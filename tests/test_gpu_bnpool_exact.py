"""Element-exact tests of the BatchNorm-affine / ReLU / 2x2 max-pool kernels (csrc/kernels/bn_pool.hip) and of the
data gradient's BatchNorm epilogue (EPI_BNBWD_BF16), on inputs full of ties inside the pooling windows and with
negative BatchNorm scales (tests/_exact.py): "the first maximum wins" is checked where maxima do tie."""
import types

import pytest
import torch

from tests import _exact as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _id(v):
    return "x".join(map(str, v))


def _dev(c, dev):
    return dict(y=c["y"].to(BF16).to(dev), g=c["g"].to(BF16).to(dev),
                **{k: c[k].to(F32).to(dev) for k in ("a", "b", "mean", "rstd")})


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_bn_apply_exact(gpu, shape, pool):
    from ddpx.ops import conv as K
    N, H, W, C = shape
    c = X.bn_case(shape, pool)
    d = _dev(c, gpu)
    out = K.bn_apply(d["y"], d["a"], d["b"], N, H, W, C, relu=True, pool=pool)
    X.assert_equal(out, X.rounded(X.bn_apply_ref(c["y"], c["a"], c["b"], pool), BF16), f"bn_apply {shape} pool {pool}")


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_bias_act_backward_exact(gpu, shape, pool):
    """a = 1, b = 0 on act = relu(conv + bias): dy IS the routed, masked gradient; dbias its integer sum."""
    from ddpx.ops import deepnn_native as D
    N, H, W, C = shape
    c = X.bn_case(shape, pool)
    act = c["y"].clamp_min(0)  # what the forward stores: many zeros and many equal maxima
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gz = X.route_ref(c["g"], act, one, zero, pool)
    plan = types.SimpleNamespace(zeros=torch.zeros(C, device=gpu), ones=torch.ones(C, device=gpu))
    g, a = c["g"].to(BF16).to(gpu), act.to(BF16).to(gpu)
    sums = gz.sum((0, 1, 2))
    for dt in (F32, BF16):
        dbias = torch.full((C,), 99.0, dtype=dt, device=gpu)
        dy = D.bias_act_backward(g, a, N, H, W, C, pool, plan, dbias=dbias)
        what = f"bias_act_backward {shape} pool {pool} {dt}"
        X.assert_equal(dy, X.rounded(gz.reshape(-1, C), BF16), what)
        X.assert_equal(dbias, X.rounded(sums, dt), what + " dbias")
        D.bias_act_backward(g, a, N, H, W, C, pool, plan, dbias=dbias, accumulate=True)
        X.assert_equal(dbias, X.rounded(sums, dt) * 2, what + " dbias accumulated")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_bn_backward_exact(gpu, shape, pool, mode):
    """dbeta / dgamma equal the float64 sums (every term is exact) under both merge kernels; dy per element within
    one bf16 ulp of the largest term of a*(gz - c1 - xhat*c2): RNE to 8 significant bits plus one possible
    rounding flip, 2^-8 * |a| * (|gz| + |c1| + |xhat*c2|).  Nothing measured."""
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    N, H, W, C = shape
    c = X.bn_case(shape, pool)
    d = _dev(c, gpu)
    dy_ref, dgamma, dbeta, terms = X.bn_backward_ref(c["g"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
    xhat = (c["y"] - c["mean"]) * c["rstd"]
    gz = X.route_ref(c["g"], c["y"], c["a"], c["b"], pool)
    assert (gz.abs() * xhat.abs()).sum((0, 1, 2)).max() * 8 < X.EXACT_LIMIT  # multiples of 1/8: sums exact in fp32
    lib = native.kernels()
    lib.ddpx_bn_set_merge(mode)
    try:
        dg = torch.full((C,), 7.0, device=gpu)
        db = torch.full((C,), 7.0, device=gpu)
        dy = K.bn_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, dgamma=dg, dbeta=db)
        dg2, db2 = dg.clone(), db.clone()
        K.bn_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, dgamma=dg2, dbeta=db2,
                      accumulate=True)
        dgb = torch.full((C,), 7.0, dtype=BF16, device=gpu)
        dbb = torch.full((C,), 7.0, dtype=BF16, device=gpu)
        K.bn_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, dgamma=dgb, dbeta=dbb)
    finally:
        lib.ddpx_bn_set_merge(-1)
    what = f"bn_backward {shape} pool {pool} merge {mode}"
    X.assert_equal(db, X.rounded(dbeta, F32), what + " dbeta")
    X.assert_equal(dg, X.rounded(dgamma, F32), what + " dgamma")
    X.assert_equal(db2, X.rounded(dbeta, F32) * 2, what + " dbeta accumulated")
    X.assert_equal(dg2, X.rounded(dgamma, F32) * 2, what + " dgamma accumulated")
    X.assert_equal(dbb, X.rounded(dbeta, BF16), what + " dbeta bf16")
    X.assert_equal(dgb, X.rounded(dgamma, BF16), what + " dgamma bf16")
    err = (dy.double().cpu().reshape(N, H, W, C) - dy_ref).abs()
    bound = terms * 2.0 ** -8
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what} dy: {int(bad.sum())} elements past one bf16 ulp of the largest term, first "
                           f"{[(tuple(i.tolist()), float(err[tuple(i)]), float(bound[tuple(i)])) for i in bad.nonzero()[:5]]}")


_DGRAD_BN_CASES = (((3, 7, 7), (64, 64)), ((2, 12, 12), (16, 24)), ((5, 16, 16), (8, 8)), ((2, 5, 3), (24, 40)))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("cfg", [8, 15, 22])
def test_conv_dgrad_bn_exact(gpu, cfg, pool):
    """The data gradient with the BatchNorm backward sums of the block below in its epilogue: g equals the plain
    data gradient, and the per-part sums add up to the exact sum of the routed gradient and of dz * xhat."""
    from ddpx.ops import conv as K
    from tests.test_gpu_conv_exact import _dev_case
    for geom, chans in _DGRAD_BN_CASES:
        N, H, W = geom
        Ci, Co = chans
        d = _dev_case(geom, chans)
        C = d["Cp"]
        assert C == Ci
        Hy, Wy = (2 * H, 2 * W) if pool else (H, W)
        bc = X.bn_case((N, Hy, Wy, C), pool, seed=1)
        bd = _dev(bc, gpu)
        g_want = X.rounded(d["dx_pad"], BF16)
        dz = X.route_ref(g_want.double(), bc["y"], bc["a"], bc["b"], pool)
        xhat = (bc["y"] - bc["mean"]) * bc["rstd"]
        assert (dz.abs() * xhat.abs()).sum((0, 1, 2)).max() * 8 < X.EXACT_LIMIT  # every partial sum exact in fp32
        assert dz.abs().sum((0, 1, 2)).max() < X.EXACT_LIMIT
        g, part = K.conv_dgrad_bn(d["dy"], d["wd"], N, H, W, C, Co, bd["y"], bd["a"], bd["b"], bd["mean"], bd["rstd"],
                                  pool, tile=cfg)
        what = f"conv_dgrad_bn {_id(geom)} {Ci}->{Co} cfg {cfg} pool {pool}"
        assert part is not None, what + ": no fused epilogue"
        pt, B = part
        X.assert_equal(g, g_want, what + " g")
        X.assert_equal(g, K.conv_dgrad(d["dy"], d["wd"], N, H, W, C, Co, tile=cfg), what + " g vs conv_dgrad")
        assert pt.shape[0] == B
        X.assert_equal(pt[:, 0].double().sum(0).cpu(), dz.sum((0, 1, 2)), what + " sum dz")
        X.assert_equal(pt[:, 1].double().sum(0).cpu(), (dz * xhat).sum((0, 1, 2)), what + " sum dz*xhat")
