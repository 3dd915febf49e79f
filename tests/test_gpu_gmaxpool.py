"""``ddpx_gmaxpool`` / ``ddpx_f32_gmaxpool`` and their backwards against the hand-written reference of
``tests/_tail_ref.py`` (checked against ``F.max_pool2d`` by ``tests/test_gmaxpool_cpu.py``): bit for bit, bf16 and
fp32, random and tied inputs, three scales."""
import pytest
import torch

from tests import _tail_ref as T

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in T.SHAPES]


def _ops(dtype):
    from ddpx.ops import conv, f32
    return conv if dtype == torch.bfloat16 else f32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", T.SHAPES, ids=IDS)
@pytest.mark.parametrize("case", ["random", "tied"])
def test_forward_and_backward_bitwise(gpu, dtype, shape, case):
    K = _ops(dtype)
    x, g = (T.random_case if case == "random" else T.tied_case)(shape, dtype, seed=7)
    xg, gg = x.to(gpu), g.to(gpu)
    for scale in T.SCALES:
        out = K.gmaxpool(xg, scale)
        gx = K.gmaxpool_backward(gg, xg, scale)
        assert out.dtype == dtype and tuple(out.shape) == (shape[0], shape[2])
        assert gx.dtype == dtype and tuple(gx.shape) == shape
        assert torch.equal(T.bits(out.cpu()), T.bits(T.gmaxpool_ref(x, scale))), (scale, "forward")
        ref = T.gmaxpool_bwd_ref(g, x, scale)
        assert torch.equal(T.bits(gx.cpu()), T.bits(ref)), (scale, "backward")
        if case == "tied":
            # exactly one non-zero entry per (n, c) column, at the lowest maximal s
            nz = gx.cpu().float() != 0
            assert torch.equal(nz.sum(1), torch.ones(shape[0], shape[2], dtype=torch.int64))
            assert torch.equal(nz.float().argmax(1), (x == x.amax(1, keepdim=True)).float().argmax(1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_four_dimensional_input_and_default_scale(gpu, dtype):
    K = _ops(dtype)
    x, g = T.random_case((4, 16, 64), dtype, seed=9)
    x4 = x.view(4, 4, 4, 64).to(gpu)
    assert torch.equal(T.bits(K.gmaxpool(x4).cpu()), T.bits(T.gmaxpool_ref(x, 1.0)))
    gx = K.gmaxpool_backward(g.to(gpu), x4)
    assert tuple(gx.shape) == (4, 4, 4, 64)
    assert torch.equal(T.bits(gx.cpu().view(4, 16, 64)), T.bits(T.gmaxpool_bwd_ref(g, x, 1.0)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_nan_in_the_window_gives_nan(gpu, dtype):
    K = _ops(dtype)
    x, _ = T.random_case((2, 5, 16), dtype, seed=2)
    x[1, 3, 7] = float("nan")
    x[0, 0, 2] = float("nan")  # the first position of a column too
    out = K.gmaxpool(x.to(gpu), 0.125).cpu()
    assert torch.isnan(out[1, 7]) and torch.isnan(out[0, 2]) and int(torch.isnan(out).sum()) == 2


def test_channel_counts_that_do_not_divide_raise(gpu):
    from ddpx.ops import conv, f32
    from ddpx.runtime import native
    err = (ValueError, native.NativeError)
    xb = torch.zeros(2, 16, 12, dtype=torch.bfloat16, device=gpu)
    xf = torch.zeros(2, 16, 6, device=gpu)
    with pytest.raises(err):
        conv.gmaxpool(xb)
    with pytest.raises(err):
        conv.gmaxpool_backward(torch.zeros(2, 12, dtype=torch.bfloat16, device=gpu), xb)
    with pytest.raises(err):
        f32.gmaxpool(xf)
    with pytest.raises(err):
        f32.gmaxpool_backward(torch.zeros(2, 6, device=gpu), xf)
    lib = native.kernels()
    out = torch.zeros(64, device=gpu)
    s = native.stream_handle()
    # the entry points themselves refuse (nothing is launched): C % 8 / C % 4, S < 1
    assert lib.ddpx_gmaxpool(xb.data_ptr(), 2, 16, 12, 1.0, out.data_ptr(), s) != 0
    assert lib.ddpx_gmaxpool_bwd(out.data_ptr(), xb.data_ptr(), 2, 16, 12, 1.0, out.data_ptr(), s) != 0
    assert lib.ddpx_f32_gmaxpool(xf.data_ptr(), 2, 16, 6, 1.0, out.data_ptr(), s) != 0
    assert lib.ddpx_f32_gmaxpool_bwd(out.data_ptr(), xf.data_ptr(), 2, 16, 6, 1.0, out.data_ptr(), s) != 0
    assert lib.ddpx_gmaxpool(xb.data_ptr(), 2, 0, 8, 1.0, out.data_ptr(), s) != 0
    assert lib.ddpx_f32_gmaxpool(xf.data_ptr(), 2, 0, 4, 1.0, out.data_ptr(), s) != 0
