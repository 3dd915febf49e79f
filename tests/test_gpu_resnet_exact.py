"""Element-exact tests of the residual additions to the BatchNorm kernels (csrc/kernels/bn_pool.hip bf16,
csrc/kernels/f32_bn.hip fp32): the skip operand of the apply pass and the second gradient of the backward, on the
exact grids of tests/_exact.py and tests/_resnet_ref.py (ties inside the pooling windows, negative scales).

The outputs are contiguous tensors, so they are placed inside a flat sentinel-filled buffer (``_slot``) and
``X.assert_guard_1d`` demands the sentinel's bits everywhere outside it; ``X.guarded`` / ``X.poisoned`` make strided
views, which these kernels (whole-tensor, contiguous NHWC) do not take.

fp32: the 4-channel window kernels serve the 8- and 64-channel shapes and the per-element kernels (the family
``DDPX_F32_BN_VEC=0`` selects everywhere) the 24-channel one, whose channel quads do not divide a workgroup.
"""
import pytest
import torch

from tests import _exact as X
from tests import _resnet_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAD = 64  # guard elements on each side of an output slot (keeps 16-B alignment for both dtypes)


def _id(v):
    return "x".join(map(str, v))


def _slot(n, dtype, dev):
    """(buffer, contiguous view of n elements in its middle), the buffer filled with the sentinel."""
    buf = torch.full((n + 2 * PAD,), X.SENTINEL[dtype], dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n]


def _check_slot(buf, n, what):
    X.assert_guard_1d(buf, PAD, PAD + n, what)
    assert not torch.isnan(buf[PAD:PAD + n]).any(), what + ": NaN in the output"


def _dev(c, dev, dt):
    """Device operands in the kernels' convention.  bf16: z = a*y + b.  fp32: z = a*(y - mean) + beta, so
    beta = b + a*mean (multiples of 1/8: exact)."""
    d = {k: c[k].to(dt).to(dev).contiguous() for k in ("y", "g", "g2", "res") if k in c}
    for k in ("a", "mean", "rstd"):
        d[k] = c[k].to(F32).to(dev)
    d["b"] = (c["b"] + c["a"] * c["mean"] if dt == F32 else c["b"]).to(F32).to(dev)
    return d


def _apply(dt, d, N, H, W, C, pool, res=None, out=None):
    if dt == BF16:
        from ddpx.ops import conv as K
        return K.bn_apply(d["y"], d["a"], d["b"], N, H, W, C, relu=True, pool=pool, res=res, out=out)
    from ddpx.ops import f32
    return f32.bn_apply(d["y"], d["a"], d["b"], d["mean"], N, H, W, C, pool, res=res, out=out)


def _backward(dt, d, N, H, W, C, pool, dgamma, dbeta, g2=None, accumulate=False, dy=None, **kw):
    if dt == BF16:
        from ddpx.ops import conv as K
        return K.bn_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, dgamma=dgamma,
                             dbeta=dbeta, accumulate=accumulate, gout2=g2, dy=dy, **kw)
    from ddpx.ops import f32
    return f32.bn_backward(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, dgamma, dbeta,
                           accumulate=accumulate, g2=g2, dy=dy, **kw)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_apply_res_exact(gpu, shape, dt):
    N, H, W, C = shape
    c = R.res_case(shape, False)
    d = _dev(c, gpu, dt)
    n = N * H * W * C
    buf, out = _slot(n, dt, gpu)
    got = _apply(dt, d, N, H, W, C, False, res=d["res"], out=out)
    want = X.rounded(R.apply_res_ref(c["y"], c["a"], c["b"], c["res"]), dt)
    X.assert_equal(got.view(N, H, W, C), want, f"bn_apply res {shape} {dt}")
    _check_slot(buf, n, f"bn_apply res {shape} {dt}")
    # res=None: the existing entry point's bits
    X.assert_equal(_apply(dt, d, N, H, W, C, False), X.rounded(X.bn_apply_ref(c["y"], c["a"], c["b"], False), dt),
                   f"bn_apply {shape} {dt}")


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_apply_res_with_pool_raises(gpu, dt):
    from ddpx.runtime.native import NativeError
    shape = X.BN_SHAPES[1]
    N, H, W, C = shape
    pc = R.res_case(shape, False)
    d = _dev(pc, gpu, dt)
    with pytest.raises(NativeError):
        _apply(dt, d, N, H, W, C, True, res=d["res"])  # refused by the entry point (-2), nothing launched
    X.assert_equal(_apply(dt, d, N, H, W, C, True), X.rounded(X.bn_apply_ref(pc["y"], pc["a"], pc["b"], True), dt),
                   "pooled apply without res")


# ------------------------------------------------------------------ backward
def _assert_dy(dy, dy_ref, terms, shape, dt, what):
    N, H, W, C = shape
    got = dy.double().cpu().reshape(N, H, W, C)
    if dt == BF16:  # tests/test_gpu_bnpool_exact.py's bound: one bf16 ulp of the largest term
        err, bound = (got - dy_ref).abs(), terms * 2.0 ** -8
        bad = ~(err <= bound)
        assert not bad.any(), (f"{what} dy: {int(bad.sum())} elements past one bf16 ulp of the largest term, first "
                               f"{[(tuple(i.tolist()), float(err[tuple(i)])) for i in bad.nonzero()[:5]]}")
    else:  # tests/test_gpu_f32.py::test_bn_relu_pool_fwd_bwd's bound
        rel = ((got - dy_ref).norm() / (dy_ref.norm() + 1e-30)).item()
        print(f"{what}: dy relative L2 error {rel:.3e}")
        assert rel < 1e-4, (what, rel)


# the merge mode belongs to the bf16 kernels: both of its settings there, fp32 once
@pytest.mark.parametrize("dt,mode", [(BF16, 0), (BF16, 1), (F32, 0)], ids=["bf16-merge0", "bf16-merge1", "fp32"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_backward_two_gradients_exact(gpu, shape, pool, mode, dt):
    """dbeta / dgamma equal the float64 sums over g1 + g2 (stored fp32, stored bf16, accumulated twice), dy within
    the one-gradient tests' bound, under both merge modes of the bf16 kernels."""
    from ddpx.runtime import native
    N, H, W, C = shape
    c = R.res_case(shape, pool)
    d = _dev(c, gpu, dt)
    dy_ref, dgamma, dbeta, terms = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"],
                                                        pool)
    R.require_exact_sums(R.route_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], pool),
                         (c["y"] - c["mean"]) * c["rstd"])
    lib = native.kernels()
    lib.ddpx_bn_set_merge(mode)
    what = f"bn_backward 2g {shape} pool {pool} merge {mode} {dt}"
    try:
        dg = torch.full((C,), 7.0, device=gpu)
        db = torch.full((C,), 7.0, device=gpu)
        buf, slot = _slot(N * H * W * C, dt, gpu)
        dy = _backward(dt, d, N, H, W, C, pool, dg, db, g2=d["g2"], dy=slot)
        dg2, db2 = dg.clone(), db.clone()
        _backward(dt, d, N, H, W, C, pool, dg2, db2, g2=d["g2"], accumulate=True)
        if dt == BF16:
            dgb = torch.full((C,), 7.0, dtype=BF16, device=gpu)
            dbb = torch.full((C,), 7.0, dtype=BF16, device=gpu)
            _backward(dt, d, N, H, W, C, pool, dgb, dbb, g2=d["g2"])
        # g2 = None: the existing entry point's bits, which are the one-gradient reference's
        dg1, db1 = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
        dy1 = _backward(dt, d, N, H, W, C, pool, dg1, db1)
    finally:
        lib.ddpx_bn_set_merge(-1)
    _check_slot(buf, N * H * W * C, what)
    X.assert_equal(db, X.rounded(dbeta, F32), what + " dbeta")
    X.assert_equal(dg, X.rounded(dgamma, F32), what + " dgamma")
    X.assert_equal(db2, X.rounded(dbeta, F32) * 2, what + " dbeta accumulated")
    X.assert_equal(dg2, X.rounded(dgamma, F32) * 2, what + " dgamma accumulated")
    if dt == BF16:
        X.assert_equal(dbb, X.rounded(dbeta, BF16), what + " dbeta bf16")
        X.assert_equal(dgb, X.rounded(dgamma, BF16), what + " dgamma bf16")
    _assert_dy(dy, dy_ref, terms, shape, dt, what)
    dy1_ref, dgamma1, dbeta1, terms1 = X.bn_backward_ref(c["g"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
    X.assert_equal(db1, X.rounded(dbeta1, F32), what + " one-gradient dbeta")
    X.assert_equal(dg1, X.rounded(dgamma1, F32), what + " one-gradient dgamma")
    _assert_dy(dy1, dy1_ref, terms1, shape, dt, what + " one-gradient")


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_backward_two_gradients_fused_sgd(gpu, shape, pool):
    """bf16 kernels: dgamma / dbeta applied as the fused SGD update equal the update made from the stored (exact)
    gradients with the kernel's own fma sequence: d = wd*p + g; d = mom*buf + d; p = p - lr*d."""
    N, H, W, C = shape
    c = R.res_case(shape, pool)
    d = _dev(c, gpu, BF16)
    _, dgamma, dbeta, _ = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
    lr, mom, wd = 0.125, 0.5, 0.25  # powers of two and small-integer gradients: every fma below is exact in fp32
    lrt = torch.tensor(lr, device=gpu)
    p0 = {k: X.ints((C,), -4, 4, 40 + i).to(F32).to(gpu) for i, k in enumerate(("gamma", "beta"))}
    m0 = {k: X.ints((C,), -4, 4, 50 + i).to(F32).to(gpu) for i, k in enumerate(("gamma", "beta"))}
    p = {k: v.clone() for k, v in p0.items()}
    m = {k: v.clone() for k, v in m0.items()}
    dy = _backward(BF16, d, N, H, W, C, pool, None, None, g2=d["g2"],
                   sgd_gamma=(p["gamma"], m["gamma"], None, lrt, mom, wd),
                   sgd_beta=(p["beta"], m["beta"], None, lrt, mom, wd))
    dg, db = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
    dy_s = _backward(BF16, d, N, H, W, C, pool, dg, db, g2=d["g2"])
    X.assert_equal(dy, dy_s, "dy with the fused update vs stored gradients")
    for k, gref in (("gamma", dgamma), ("beta", dbeta)):
        g64 = gref.to(gpu)
        buf = mom * m0[k].double() + (wd * p0[k].double() + g64)
        X.assert_equal(m[k], buf.float(), f"fused SGD momentum {k} {shape} pool {pool}")
        X.assert_equal(p[k], (p0[k].double() - lr * buf).float(), f"fused SGD parameter {k} {shape} pool {pool}")


class _MirrorComm:
    """The 2-rank communicator of tests/test_gpu_vgg.py whose other rank holds this rank's data."""
    world_size = 2
    rank = 0

    def allgather(self, out, inp, stream=None):
        out.view(2, -1).copy_(inp.view(1, -1).expand(2, -1))

    def allreduce_(self, t, op="sum", stream=None, async_op=False):
        assert op == "sum"
        t.mul_(2.0)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=_id)
def test_backward_two_gradients_sync_split(gpu, shape, pool, dt):
    """The SyncBatchNorm split (sums -> all-reduce -> apply) over a mirror communicator: 2 x sums / (2 M) are the
    local means bit for bit (a power-of-two scale), so dy equals the one-call path's and dgamma / dbeta stay the
    local exact sums."""
    N, H, W, C = shape
    c = R.res_case(shape, pool)
    d = _dev(c, gpu, dt)
    _, dgamma, dbeta, _ = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
    dg, db, dgs, dbs = (torch.empty(C, device=gpu) for _ in range(4))
    dy = _backward(dt, d, N, H, W, C, pool, dg, db, g2=d["g2"])
    if dt == BF16:
        from ddpx.ops import conv as K
        dys = K.bn_backward_sync(d["g"], d["y"], d["a"], d["b"], d["mean"], d["rstd"], N, H, W, C, pool, _MirrorComm(),
                                 dgamma=dgs, dbeta=dbs, gout2=d["g2"])
    else:
        dys = _backward(dt, d, N, H, W, C, pool, dgs, dbs, g2=d["g2"], comm=_MirrorComm())
    X.assert_equal(dgs, X.rounded(dgamma, F32), "sync dgamma")
    X.assert_equal(dbs, X.rounded(dbeta, F32), "sync dbeta")
    M = N * H * W
    if dt == BF16 and (M & (M - 1)):
        # sums * (1 / (2M)) instead of sums / M: the means differ by an fp32 rounding, dy by at most a bf16 ulp
        _, _, _, terms = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
        err = (dys.double() - dy.double()).abs().cpu().reshape(N, H, W, C)
        assert (err <= terms * 2.0 ** -7).all(), float(err.max())
    else:
        X.assert_equal(dys, dy, f"sync dy {shape} pool {pool} {dt}")


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("pool", [False, True])
def test_gradient_sum_is_not_rounded(gpu, pool, dt):
    """g1 from {-64, 64}, g2 from {-0.25, 0.25}: 64.25 needs 9 significant bits; a kernel that rounded g1 + g2 to
    bf16 would sum +-64 and miss the exact dbeta / dgamma (tests/test_resnet_cpu.py shows the two differ)."""
    shape = X.BN_SHAPES[-1]
    N, H, W, C = shape
    c = R.unrounded_case(shape, pool)
    d = _dev(c, gpu, dt)
    xhat = (c["y"] - c["mean"]) * c["rstd"]
    R.require_exact_sums(R.route_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], pool), xhat, g_unit=4, x_unit=8)
    dy_ref, dgamma, dbeta, terms = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"],
                                                        pool)
    dg, db = torch.empty(C, device=gpu), torch.empty(C, device=gpu)
    dy = _backward(dt, d, N, H, W, C, pool, dg, db, g2=d["g2"])
    X.assert_equal(db, X.rounded(dbeta, F32), f"unrounded sum dbeta pool {pool} {dt}")
    X.assert_equal(dg, X.rounded(dgamma, F32), f"unrounded sum dgamma pool {pool} {dt}")
    _assert_dy(dy, dy_ref, terms, shape, dt, f"unrounded sum pool {pool} {dt}")
