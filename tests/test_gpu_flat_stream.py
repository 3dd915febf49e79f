"""The one streaming loop of the flat optimizer kernels (``stream2``, ``csrc/include/ddpx_flat_optim.h``): an update
does not depend on how the loop cuts its range.

The chunk-driven form (``first = blockIdx.y * 256 + tid``, ``stride = gridDim.y * 256``): one step from identical
inputs with 1, 2, 4 and 8 workgroups per chunk must give the same bits in master, every state buffer and the bf16
shadow, and must leave every padding element between parameters alone.  The parameters' numels sit on the loop's edges
(16-B vectors ``nv = numel // 4`` per chunk of at most 32768 elements, ``stride = 256 * split`` vectors):

    3                    tail only, no vector
    5                    one vector + a tail of 1
    1021, 1024, 1029     nv = 255, 256, 257: around one workgroup's first pass
    2049                 nv = 512 + a tail of 1
    4100, 8195, 16389    just past stride resp. 2 * stride for splits 2, 4 and 8
    32768                a full chunk
    32771                a full chunk + a 3-element chunk
    65541                two full chunks + a short chunk with a tail

The flat form (``first = blockIdx.x * 256 + tid``, ``stride`` = the capped grid's threads ``T``): over
``n = 2 T 4 + 4 * 256 + 3`` elements the loop's second pass has a region with two vectors in flight, a region with
one, and a scalar tail; the result must be, bit for bit, the same kernel run piecewise over ``[0, n1)`` and
``[n1, n)``, whose small first piece moves every later element to another thread, pass and slot.
"""
import pytest
import torch

from tests.test_gpu_param_groups import _Odd, _bc, _bits, _hyper

pytestmark = pytest.mark.gpu

NUMELS = [3, 5, 1021, 1024, 1029, 2049, 4100, 8195, 16389, 32768, 32771, 65541]
SPLITS = (1, 2, 4, 8)
GD = pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
BETAS, EPS = (0.9, 0.999), 1e-8
SENTINEL = 3.0  # exact in fp32 and bf16


def _store(gpu, grad_dtype):
    """The store of NUMELS with random gradients and states and SENTINEL in every padding element of master, shadow
    and the states; returns ``(flat, pad, states)``."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(11)
    flat = FlatParams(_Odd([(n,) for n in NUMELS]).to(gpu), grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)
    assert sorted(flat.numels) == NUMELS
    pad = torch.ones(flat.total, dtype=torch.bool, device=gpu)
    for o, n in zip(flat.offsets, flat.numels):
        pad[o:o + n] = False
    assert pad.any()
    st = {"momentum": torch.randn(flat.total, device=gpu) * 0.05, "exp_avg": torch.randn(flat.total, device=gpu) * 0.01,
          "exp_avg_sq": (torch.randn(flat.total, device=gpu) * 0.01).square()}
    flat.grad.copy_(torch.randn(flat.total, device=gpu) * 0.5)
    flat.shadow.copy_(flat.master)
    for t in (flat.master, flat.shadow, *st.values()):
        t[pad] = SENTINEL
    return flat, pad, st


def _tables(flat, gpu):
    """A trust table with a different ratio per parameter and a hyper table with two row values."""
    P = len(flat.params)
    trust = torch.linspace(0.5, 2.0, P, device=gpu)
    hyper = _hyper(flat, [1.0 if i % 2 else 0.25 for i in range(P)], [5e-4 if i % 2 else 0.0 for i in range(P)])
    return trust, hyper


def _sgd(flat, st, bc, trust, hyper):
    from ddpx.ops.lars import LarsPlan
    plan = LarsPlan(flat)
    plan.trust_dev.copy_(trust)
    plan.update(0, flat.total, 0.4, 0.9, 5e-4, momentum_buf=st["momentum"], hyper=hyper)


def _adamw(flat, st, bc, trust, hyper):
    from ddpx.ops.lars import PidChunkPlan
    PidChunkPlan(flat).adamw_update(0, flat.total, hyper, 1e-2, st["exp_avg"], st["exp_avg_sq"], bc, *BETAS, EPS)


def _lamb_apply(flat, st, bc, trust, hyper):
    from ddpx.ops.lamb import LambPlan
    plan = LambPlan(flat)
    plan.trust_dev.copy_(trust)
    plan.apply(0, flat.total, 1e-2, st["exp_avg"], st["exp_avg_sq"], bc, 1e-6, 5e-4, hyper=hyper)


# (the update, its split knob, whether it also runs without the hyper table, the state buffers it writes)
CHUNK_KERNELS = {
    "sgd": (_sgd, "ddpx_lars_set_split", True, ("momentum",)),
    "adamw": (_adamw, "ddpx_adamw_set_split", False, ("exp_avg", "exp_avg_sq")),
    "lamb_apply": (_lamb_apply, "ddpx_lamb_set_split", True, ()),
}


@GD
@pytest.mark.parametrize("kernel", list(CHUNK_KERNELS))
def test_chunk_driven_update_does_not_depend_on_the_split(gpu, grad_dtype, kernel):
    from ddpx.runtime import native
    run, knob, without_table, written = CHUNK_KERNELS[kernel]
    set_split = getattr(native.kernels(), knob)
    flat, pad, st = _store(gpu, grad_dtype)
    trust, hyper = _tables(flat, gpu)
    bc = _bc(gpu)
    bufs = {"master": flat.master, "shadow": flat.shadow, **st}
    start = {k: t.clone() for k, t in bufs.items()}
    g0 = flat.grad.clone()
    default = set_split(0)  # not a split: only returns the value in force
    assert default in SPLITS
    try:
        for h in ((None, hyper) if without_table else (hyper,)):
            outs = []
            for split in SPLITS:
                assert set_split(split) == split
                for k, t in bufs.items():
                    t.copy_(start[k])
                run(flat, st, bc, trust, h)
                outs.append({k: t.clone() for k, t in bufs.items()})
            for split, out in zip(SPLITS, outs):
                for k in bufs:
                    what = (kernel, h is not None, split, k)
                    assert torch.equal(_bits(out[k]), _bits(outs[0][k])), what
                    assert torch.equal(_bits(out[k])[pad], _bits(start[k])[pad]), (*what, "padding was written")
                    changed = (_bits(out[k]) != _bits(start[k]))[~pad].float().mean().item()
                    if k == "master" or k in written:
                        assert changed > 0.99, (*what, "not updated", changed)
                    elif k != "shadow":
                        assert changed == 0.0, what
                assert torch.equal(out["shadow"][~pad], out["master"][~pad].to(torch.bfloat16)), (kernel, split)
    finally:
        assert set_split(default) == default
    assert torch.equal(_bits(flat.grad), _bits(g0))


@GD
@pytest.mark.parametrize("kernel", ["sgd", "adamw"])
def test_flat_grid_stride_update_does_not_depend_on_the_cut(gpu, grad_dtype, kernel):
    from ddpx.ops.elementwise import adamw_flat_, sgd_flat_
    from ddpx.runtime import native
    T = native.kernels().ddpx_ema_max_threads()
    assert T == 2048 * 256
    n = 2 * T * 4 + 4 * 256 + 3
    n1 = 4 * 1000
    assert n1 % 4 == 0 and n1 < T * 4 // 100
    gen = torch.Generator(device=gpu).manual_seed(12)
    p0 = torch.randn(n, device=gpu, generator=gen) * 0.1
    a0 = torch.randn(n, device=gpu, generator=gen) * 0.05
    b0 = (torch.randn(n, device=gpu, generator=gen) * 0.01).square()
    g = (torch.randn(n, device=gpu, generator=gen) * 0.5).to(grad_dtype)
    s0 = torch.zeros(n, dtype=torch.bfloat16, device=gpu)
    bc = _bc(gpu)

    def step(p, a, b, grad, s):
        if kernel == "sgd":
            sgd_flat_(p, a, grad, s, 0.4, 0.9, 5e-4)
        else:
            adamw_flat_(p, a, b, grad, s, 1e-2, bc, None, *BETAS, EPS, 0.01)

    whole = [t.clone() for t in (p0, a0, b0, s0)]
    step(whole[0], whole[1], whole[2], g, whole[3])
    pieces = [t.clone() for t in (p0, a0, b0, s0)]
    for lo, hi in ((0, n1), (n1, n)):
        step(pieces[0][lo:hi], pieces[1][lo:hi], pieces[2][lo:hi], g[lo:hi], pieces[3][lo:hi])
    for name, x, y in zip(("p", "state 0", "state 1", "shadow"), whole, pieces):
        assert torch.equal(_bits(x), _bits(y)), (kernel, name)
    assert (_bits(whole[0]) != _bits(p0)).float().mean().item() > 0.99
    assert torch.equal(whole[3], whole[0].to(torch.bfloat16))
