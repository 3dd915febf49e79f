"""The two kernels of a pre-activation residual block: the shortcut add with the BatchNorm statistics of the sum
(csrc/kernels/bn_preact.hip) and the BatchNorm backward with the skip gradient added on its output side
(``bn_backward(gadd=)``, csrc/kernels/bn_pool.hip), against tests/_preact_ref.py."""
import pytest
import torch

from tests import _exact as X
from tests import _preact_ref as P

pytestmark = pytest.mark.gpu

F32, BF16, I16, I32 = torch.float32, torch.bfloat16, torch.int16, torch.int32
# one group; a short last tile; odd extents and a group count that does not divide the block; 2 tiles of 32 rows
# exactly; the widest case; 5 tiles; 520 tiles of 128 rows exactly (past 65536 rows a tile has 128 rows, not 32)
SHAPES = ((1, 1, 1, 8), (2, 3, 5, 8), (5, 7, 7, 24), (3, 4, 4, 64), (4, 4, 4, 16), (2, 8, 8, 512), (9, 4, 4, 512),
          (65, 32, 32, 64))


def _operands(shape, gpu):
    g = torch.Generator().manual_seed(sum(shape))
    M, C = shape[0] * shape[1] * shape[2], shape[3]
    return ((torch.randn(M, C, generator=g) * 2 + 0.5).to(BF16).to(gpu),
            (torch.randn(M, C, generator=g) * 3 - 1).to(BF16).to(gpu))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_preact_add(gpu, shape):
    """Training: z bit for bit (also in y's storage); mean / rstd / running statistics after bn_finalize against
    float64 statistics of the stored z within tests/test_gpu_vgg.py::test_bn_merges_match_fp64's bounds for the
    convolution epilogue's statistics (mean 1e-5 / 1e-5, rstd and running variance 1e-4 / 1e-5); two launches, the
    same bits.  Evaluation, one pass: the same z, and act bit-equal to bn_apply on the stored z."""
    from ddpx.ops import conv as K
    N, H, W, C = shape
    M = N * H * W
    y, s = _operands(shape, gpu)
    want = (y.float() + s.float()).to(BF16)  # the fp32 sum, rounded once
    z, st, T, BM = K.preact_add(y, s, N, H, W, C)
    assert BM == (32 if M <= 65536 else 128) and T == -(-M // BM) and tuple(st.shape) == (T, 2, C)
    assert torch.equal(z.view(I16), want.view(I16))
    assert torch.equal(K.preact_add(y, s, N, H, W, C)[1].view(I32), st.view(I32))
    ya = y.clone()
    za, sta, _, _ = K.preact_add(ya, s, N, H, W, C, out=ya)
    assert za.data_ptr() == ya.data_ptr() and torch.equal(ya.view(I16), want.view(I16))
    assert torch.equal(sta.view(I32), st.view(I32))
    bn = torch.nn.BatchNorm2d(C).to(gpu)
    a, b, mean, rstd = (torch.empty(C, device=gpu) for _ in range(4))
    K.bn_finalize(st, T, BM, M, bn, True, a, b, mean, rstd)
    z64 = want.double()
    mean64, var64, unb64 = z64.mean(0), z64.var(0, unbiased=False), z64.var(0, unbiased=M > 1)
    assert torch.allclose(mean.double(), mean64, rtol=1e-5, atol=1e-5)
    assert torch.allclose(rstd.double(), (var64 + 1e-5).rsqrt(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(bn.running_mean.double(), 0.1 * mean64, rtol=1e-5, atol=1e-5)
    assert torch.allclose(bn.running_var.double(), 0.9 + 0.1 * unb64, rtol=1e-4, atol=1e-5)
    assert int(bn.num_batches_tracked) == 1
    z, act = K.preact_add(y, s, N, H, W, C, stats=False, eval_ab=(a, b))
    assert torch.equal(z.view(I16), want.view(I16)) and tuple(act.shape) == (N, H, W, C)
    assert torch.equal(act.view(I16), K.bn_apply(z, a, b, N, H, W, C).view(I16))
    with pytest.raises(ValueError, match="one of them"):
        K.preact_add(y, s, N, H, W, C, eval_ab=(a, b))


def _dev(c, gpu):
    return [c[k].to(BF16 if k in ("y", "g") else F32).to(gpu) for k in ("g", "y", "a", "b", "mean", "rstd")]


def _check(dy, dg, db, ref, what):
    """tests/test_gpu_bnpool_exact.py::test_bn_backward_exact's checks: dgamma / dbeta equal the float64 sums, dy
    within 2^-8 * terms, one bf16 ulp of its terms' magnitudes; gadd is one more term (tests/_preact_ref.py)."""
    dy_ref, dgamma, dbeta, terms = ref
    X.assert_equal(db, X.rounded(dbeta, F32), what + " dbeta")
    X.assert_equal(dg, X.rounded(dgamma, F32), what + " dgamma")
    err = (dy.double().cpu().reshape(dy_ref.shape) - dy_ref).abs()
    bad = ~(err <= terms * 2.0 ** -8)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements past the bound, largest error {float(err.max())}"


@pytest.mark.parametrize("shape", SHAPES[:-1], ids=str)  # the apply pass has one path: nothing new at 66560 rows
def test_bn_backward_gadd(gpu, shape):
    from ddpx.ops import conv as K
    C = shape[3]
    c = X.bn_case(shape, False)
    args = (*_dev(c, gpu), *shape, False)
    gadd = X.ints(shape, -3, 3, 77 + C)
    ga = gadd.reshape(-1, C).to(BF16).to(gpu)
    dg0, db0, dg1, db1 = (torch.full((C,), 7.0, device=gpu) for _ in range(4))
    plain = K.bn_backward(*args, dgamma=dg0, dbeta=db0)
    dy = K.bn_backward(*args, dgamma=dg1, dbeta=db1, gadd=ga)
    _check(dy, dg1, db1, P.bn_backward_add_ref(c, gadd), f"bn_backward gadd {shape}")
    assert torch.equal(dg0.view(I32), dg1.view(I32)) and torch.equal(db0.view(I32), db1.view(I32))
    # x + 0 is x for every x but -0, which torch.equal takes for +0 (tests/_exact.py's convention)
    assert torch.equal(K.bn_backward(*args, dgamma=dg1, dbeta=db1, gadd=torch.zeros_like(ga)), plain)
    with pytest.raises(ValueError, match="gout2"):
        K.bn_backward(*args, dgamma=dg1, dbeta=db1, gadd=ga, gout2=args[0])
    with pytest.raises(ValueError, match="pool"):
        K.bn_backward(*args[:-1], True, dgamma=dg1, dbeta=db1, gadd=ga)


def test_bn_backward_gadd_from_dgrad_sums(gpu):
    """The tail path: the sums come from the data gradient's epilogue (a tile with a fused variant), gadd is added
    by the apply pass behind the merge."""
    from ddpx.ops import conv as K
    from tests.test_gpu_conv_exact import _dev_case
    (N, H, W), (Ci, Co) = (3, 7, 7), (64, 64)
    d = _dev_case((N, H, W), (Ci, Co))
    c = dict(X.bn_case((N, H, W, Ci), False, seed=1))
    bn = _dev(c, gpu)[1:]
    g, part = K.conv_dgrad_bn(d["dy"], d["wd"], N, H, W, Ci, Co, *bn, False, tile=8)
    assert part is not None
    c["g"] = g.double().cpu()
    gadd = X.ints((N, H, W, Ci), -3, 3, 5)
    dg, db = torch.empty(Ci, device=gpu), torch.empty(Ci, device=gpu)
    dy = K.bn_backward(g, *bn, N, H, W, Ci, False, dgamma=dg, dbeta=db, part=part,
                       gadd=gadd.reshape(-1, Ci).to(BF16).to(gpu))
    _check(dy, dg, db, P.bn_backward_add_ref(c, gadd), "bn_backward part= gadd")
