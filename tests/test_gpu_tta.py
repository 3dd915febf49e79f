"""Flip test-time augmentation: the mirror kernel against ``torch.flip``, the metrics launch with a second logits
operand against the fp64 twin (the rules of ``tests/test_gpu_eval_metrics.py``: exact counts, the loss sum within
``1e-5 * rows``), and ``evaluate_metrics(tta_flip=True)`` on symmetric and on random images."""
import numpy as np
import pytest
import torch

from ddpx.ops.head import EvalAccumulator, eval_metrics
from tests._eval_ref import gaussian_logits, grid_logits, ref_metrics
from tests._tail_ref import bits

pytestmark = pytest.mark.gpu

# tests/test_gpu_eval_metrics.py's bound: the mean's one rounded add (at most 4.8e-7 at |z| <= 8) is below the few 1e-6
# a row carries there
LOSS_TOL = 1e-5
HFLIP_LAYOUTS = ["nchw_f32", "nchw_bf16", "flat_f32", "flat_bf16", "nhwc_bf16", "nhwc_f32", "nhwc8_bf16", "nhwc4_f32"]


def _batch(layout, N, size, seed=0):
    """A random batch in ``layout`` and the axis of its image width (None: flat)."""
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if "bf16" in layout else torch.float32
    if layout.startswith("flat"):
        return torch.randn(N, 3 * size * size, generator=g).to(dt), None
    if layout.startswith("nchw"):
        return torch.randn(N, 3, size, size, generator=g).to(dt), 3
    C = {"nhwc8_bf16": 8, "nhwc4_f32": 4}.get(layout, 3)
    return torch.randn(N, size, size, C, generator=g).to(dt), 2


@pytest.mark.parametrize("size", [16, 32])
@pytest.mark.parametrize("layout", HFLIP_LAYOUTS)
def test_hflip_equals_torch_flip(gpu, layout, size):
    from ddpx.ops.elementwise import hflip
    x, axis = _batch(layout, 3, size)
    want = x.view(3, 3, size, size).flip(3).reshape(x.shape) if axis is None else x.flip(axis)
    got = hflip(x.to(gpu), layout, width=size)
    assert got.dtype == x.dtype and got.shape == x.shape
    assert torch.equal(bits(got.cpu()), bits(want.contiguous()))
    assert torch.equal(bits(hflip(got, layout, width=size).cpu()), bits(x))  # an involution
    assert torch.equal(bits(hflip(x, layout, width=size)), bits(want.contiguous()))  # the CPU form


def test_hflip_odd_width_and_bad_arguments(gpu):
    from ddpx.ops.elementwise import hflip
    from ddpx.runtime import native
    x = torch.randn(2, 3, 5, 7)  # no 16-B row: the unit-by-unit kernel
    assert torch.equal(hflip(x.to(gpu), "nchw_f32").cpu(), x.flip(3))
    xb = x.to(torch.bfloat16)
    assert torch.equal(bits(hflip(xb.to(gpu), "nchw_bf16").cpu()), bits(xb.flip(3).contiguous()))
    with pytest.raises(ValueError):
        hflip(x.to(gpu), "nchw_bf16")
    with pytest.raises(ValueError):
        hflip(x.to(gpu), "nope")
    flat = torch.randn(2, 3 * 4 * 8, device=gpu)  # 4x8 images: no square, so the width has to be given
    with pytest.raises(ValueError, match="pass width"):
        hflip(flat, "flat_f32")
    assert torch.equal(hflip(flat, "flat_f32", width=8), flat.view(2, 3, 4, 8).flip(3).reshape(2, -1))
    lib = native.kernels()
    d = x.to(gpu)
    out = torch.empty_like(d)
    s = native.stream_handle()
    assert lib.ddpx_hflip(d.data_ptr(), 30, 7, 3, out.data_ptr(), s) != 0   # odd element size
    assert lib.ddpx_hflip(d.data_ptr(), 30, 7, 4, d.data_ptr(), s) != 0     # in place


# ------------------------------------------------------------------ the second logits operand
def _two(kind, M, C):
    f = gaussian_logits if kind == "gaussian" else grid_logits
    z1, t = f(M, C, seed=M * 1000 + C)
    z2, _ = f(M, C, seed=M * 1000 + C + 1)
    return z1, z2, t


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("C,k", [(10, 1), (10, 5), (100, 5)])
def test_two_operands_equal_the_fp64_twin(gpu, C, k, kind):
    M = 37
    z1, z2, t = _two(kind, M, C)
    mean = 0.5 * (z1.astype(np.float64) + z2.astype(np.float64))
    for mv in (M, 19):
        acc = EvalAccumulator(gpu)
        eval_metrics(torch.from_numpy(z1).to(gpu), torch.from_numpy(t).to(gpu), acc, k, mv,
                     logits2=torch.from_numpy(z2).to(gpu))
        loss, h1, hk, rows, _ = ref_metrics(mean, t, k, mv)
        got = acc.read()
        print(f"C {C} k {k} {kind} m_valid {mv}: loss {got[0]:.9f} ref {loss:.9f} counts {got[1:]}")
        assert got[1:] == (h1, hk, rows), (got, (h1, hk, rows))
        assert abs(got[0] - loss) <= LOSS_TOL * max(rows, 1), (got[0], loss)
        # the CPU twin of eval_metrics does the same in fp64
        cpu = EvalAccumulator("cpu")
        eval_metrics(torch.from_numpy(z1), torch.from_numpy(t), cpu, k, mv, logits2=torch.from_numpy(z2))
        cgot = cpu.read()
        assert cgot[1:] == (h1, hk, rows) and abs(cgot[0] - loss) <= 1e-9 * max(rows, 1)


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("C,k", [(10, 5), (100, 5)])
def test_the_same_operand_twice_is_the_one_operand_launch(gpu, C, k, kind):
    z, _, t = _two(kind, 37, C)
    zg, tg = torch.from_numpy(z).to(gpu), torch.from_numpy(t).to(gpu)
    one, two = EvalAccumulator(gpu), EvalAccumulator(gpu)
    eval_metrics(zg, tg, one, k)
    eval_metrics(zg, tg, two, k, logits2=zg)
    assert torch.equal(one.counts, two.counts) and torch.equal(bits(one.loss_sum.float()), bits(two.loss_sum.float()))
    assert torch.equal(one.loss_sum, two.loss_sum)
    # a row stride wider than the classes, shared by both operands
    wide = torch.full((37, C + 7), float("nan"), device=gpu)
    wide[:, :C] = zg
    three = EvalAccumulator(gpu)
    eval_metrics(wide[:, :C], tg, three, k, logits2=wide[:, :C])
    assert torch.equal(one.counts, three.counts) and torch.equal(one.loss_sum, three.loss_sum)


def test_second_operand_must_match(gpu):
    z = torch.zeros(4, 10, device=gpu)
    t = torch.zeros(4, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        eval_metrics(z, t, EvalAccumulator(gpu), 1, logits2=torch.zeros(4, 9, device=gpu))
    with pytest.raises(ValueError):
        eval_metrics(z, t, EvalAccumulator(gpu), 1, logits2=torch.zeros(4, 10))


# ------------------------------------------------------------------ evaluate_metrics(tta_flip=True)
def _model(gpu, name):
    import ddpx
    from ddpx.models import MLP, ResNet9
    torch.manual_seed(6)
    if name == "mlp":
        m = MLP(hidden=256)
        layout = "flat_bf16"
    else:
        m = ResNet9(tail="max", tail_scale=0.125)
        m.use_native, m.native_dtype = True, "bf16"
        layout = "nhwc8_bf16"
    ddpx.prepare_model(m, gpu)
    return m, layout


def _to_layout(x, layout):
    """An NCHW fp32 batch in the loader's ``layout``, as the augment kernel writes an unaugmented batch."""
    if layout == "flat_bf16":
        return x.reshape(x.shape[0], -1).to(torch.bfloat16)
    assert layout == "nhwc8_bf16"
    return torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, 5)).to(torch.bfloat16).contiguous()


@pytest.mark.parametrize("name", ["mlp", "resnet9"])
def test_evaluate_metrics_with_flip_tta(gpu, name):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.train.evaluate import evaluate_metrics
    m, layout = _model(gpu, name)
    # left-right symmetric images: the mirror image is the image, so the numbers are the plain evaluation's exactly
    sym = synthetic_cifar(70, seed=8)
    sym.images[..., 16:] = sym.images[..., :16].flip(-1)
    loader = DeviceLoader(sym, 32, gpu, train=False, layout=layout)
    plain = evaluate_metrics(m, loader, topk=5, progress=False)
    tta = evaluate_metrics(m, loader, topk=5, progress=False, tta_flip=True)
    assert tta == plain and plain.samples == 70 and plain.loss == plain.loss
    assert m.training
    # random images: a torch composition that flips the NCHW batch
    ds = synthetic_cifar(70, seed=9)
    loader = DeviceLoader(ds, 32, gpu, train=False, layout=layout)
    nchw = DeviceLoader(ds, 32, gpu, train=False, layout="nchw_f32")
    got = evaluate_metrics(m, loader, topk=5, progress=False, tta_flip=True)
    ref = EvalAccumulator("cpu")
    m.eval()
    with torch.inference_mode():
        for x, y in nchw:
            z1 = m(_to_layout(x, layout)).float().cpu()
            z2 = m(_to_layout(x.flip(3), layout)).float().cpu()
            eval_metrics(z1, y.cpu(), ref, 5, logits2=z2)
    m.train()
    loss_sum, h1, hk, rows = ref.read()
    print(f"{name}: tta loss {got.loss:.7f} ref {loss_sum / rows:.7f} top1 {got.top1} top5 {got.topk}")
    assert rows == got.samples == 70
    assert got.top1 == h1 / rows * 100 and got.topk == hk / rows * 100
    assert abs(got.loss * rows - loss_sum) <= LOSS_TOL * rows
    assert got != evaluate_metrics(m, loader, topk=5, progress=False)  # the second forward counts
