"""LARS on the GPU: the per-parameter sum-of-squares kernels, the trust table, ``ddpx_sgd_flat_chunks`` against
``ddpx_sgd_flat`` and against fp64, ``ddpx.optim.LARS`` eager against captured, under replicated DDP, on a whole
model and through a full checkpoint.

Tolerances, all counted from the kernels' rounding sequences (``csrc/kernels/lars.hip``); u = 2^-24.

* Sums of squares: ``tests/test_gpu_clip.py``'s ``BOUND`` (44 u).  ``ddpx_lars_sumsq`` has ``grad_sumsq_kernel``'s
  accumulator shape for w^2 and for g^2, and ``ddpx_lars_segment_reduce`` ends, like ``sumsq_reduce_kernel``, with
  one rounding of an fp64 total.  A total completed by a second, accumulating reduction is rounded twice: + u.
* Trust ratio from the fp32 totals the kernel read (``K_T`` = 7 u, every term >= 0, no cancellation):
  wn = sqrt (1), trust_coef * wn (1): numerator 2 u.  gn = sqrt (1), c * gn (1, clipped only); the denominator
  fma(wd, wn, gn) + eps carries its inputs' larger error (2 u) + the fma (1) + the add (1): 4 u.  The division: 1.
* Clip factor from the fp32 sum of the g^2 totals: sqrt, + 1e-6, the division: 3 u (``K_C``).
* The update, one launch and several steps: ``tests/_lars_ref.py``.
"""
import math

import pytest
import torch

from tests._lars_ref import SUMSQ, U, LarsFp64, f32

pytestmark = pytest.mark.gpu

BOUND = SUMSQ
K_T, K_C = 7, 3
HP = dict(lr=0.4, momentum=0.9, weight_decay=5e-4, trust_coef=1e-3, eps=1e-8)


def _shapes():
    """The odd sizes [1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 5, 2 * CHUNK + 1], some as 2-D tensors."""
    from ddpx.ops.clip import CHUNK
    assert CHUNK == 32768
    return [(1,), (3,), (2, 2), (7, 9), (64,), (5, 13), (7, 4681), (128, 256), (CHUNK + 5,), (2 * CHUNK + 1, 1)]


class _Odd(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s) * 0.1) for s in shapes])


def _pad_mask(flat):
    pad = torch.ones(flat.total, dtype=torch.bool, device=flat.device)
    for o, n in zip(flat.offsets, flat.numels):
        pad[o:o + n] = False
    return pad


def _store(gpu, grad_dtype, seed=0):
    """A flat store over the odd-shaped parameters, random gradients and momentum, and NaN in every padding element
    of gradient, master, momentum and shadow."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m = _Odd(_shapes()).to(gpu)
    flat = FlatParams(m, grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)
    pad = _pad_mask(flat)
    assert pad.any()
    mom = torch.randn(flat.total, device=gpu) * 0.05
    nan = float("nan")
    flat.master[pad] = nan
    flat.shadow[pad] = nan
    mom[pad] = nan
    _fill(flat, seed)
    return m, flat, pad, mom


def _fill(flat, seed, scale=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat.grad.fill_(float("nan"))
    for p in flat.params:
        p.main_grad.copy_((torch.randn(p.shape, generator=g) * scale).to(flat.device))
        flat.grad_done(p)


def _still_nan(pad, *tensors):
    for t in tensors:
        assert torch.isnan(t[pad].float()).all(), "a padding element was written"


def _ref_sq(flat):
    w = [flat.master[flat.slice(i)].double().square().sum().item() for i in range(len(flat.params))]
    g = [flat.grad[flat.slice(i)].double().square().sum().item() for i in range(len(flat.params))]
    return w, g


GD = pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])


@GD
def test_per_parameter_sums_of_squares(gpu, grad_dtype):
    from ddpx.ops.lars import LarsPlan
    _, flat, pad, _ = _store(gpu, grad_dtype)
    P = len(flat.params)
    plan = LarsPlan(flat)
    plan.compute(**{k: HP[k] for k in ("trust_coef", "weight_decay", "eps")})
    sq1, part1 = plan.sq.clone(), plan.partials_buf.clone()
    assert torch.isfinite(sq1).all(), "NaN padding leaked into a sum"
    rw, rg = _ref_sq(flat)
    worst = 0.0
    for i in range(P):
        for got, want in ((sq1[i].item(), rw[i]), (sq1[P + i].item(), rg[i])):
            worst = max(worst, abs(got - want) / want)
            assert abs(got - want) <= BOUND * want, (i, got, want)
    # chunk by chunk (a wrong chunk cannot hide in a total), and every chunk inside its parameter
    for (s, n, pid), (pw, pg) in zip(plan.chunks, part1.cpu().tolist()):
        assert flat.offsets[pid] <= s and s + n <= flat.offsets[pid] + flat.numels[pid]
        ww = flat.master[s:s + n].double().square().sum().item()
        wg = flat.grad[s:s + n].double().square().sum().item()
        assert abs(pw - ww) <= BOUND * ww and abs(pg - wg) <= BOUND * wg, (s, n)
    print(f"sumsq {grad_dtype}: worst relative error {worst:.3e} (bound {BOUND:.3e})")
    # a second call: the same bits
    plan.partials_buf.zero_()
    plan.sq.zero_()
    plan.compute(**{k: HP[k] for k in ("trust_coef", "weight_decay", "eps")})
    assert torch.equal(plan.sq, sq1) and torch.equal(plan.partials_buf, part1)
    # two shards that cut the biggest parameter at a 64-element boundary, the second accumulated onto the first
    big = max(range(P), key=lambda i: flat.numels[i])
    cut = flat.offsets[big] + 64 * 517
    split = LarsPlan(flat, [(0, cut), (cut, flat.total)])
    split.partials(1)
    split.partials(0)
    split.reduce(span=(0, 1))
    after = [i for i in range(P) if flat.offsets[i] >= cut]
    assert after and all(split.sq[i].item() == 0 and split.sq[P + i].item() == 0 for i in after)
    split.reduce(accumulate=True, span=(1, 2))
    for i in range(P):
        for got, want in ((split.sq[i].item(), rw[i]), (split.sq[P + i].item(), rg[i])):
            assert abs(got - want) <= (BOUND + U) * want, (i, got, want)
        if i != big:  # one piece: the same chunks, the same bits
            assert split.sq[i] == sq1[i] and split.sq[P + i] == sq1[P + i]


def _want_trust(sq, plain, P, hp, coef):
    tc, wd, eps = f32(hp["trust_coef"]), f32(hp["weight_decay"]), f32(hp["eps"])
    out = []
    for i in range(P):
        wn, gn = math.sqrt(sq[i]), coef * math.sqrt(sq[P + i])
        adapt = (not plain[i]) and wn > 0 and gn > 0
        out.append(tc * wn / (gn + wd * wn + eps) if adapt else 1.0)
    return out


@GD
@pytest.mark.parametrize("max_norm", [None, 5.0], ids=["noclip", "clip"])
def test_trust_table(gpu, grad_dtype, max_norm):
    from ddpx.ops.lars import LarsPlan
    m, flat, pad, _ = _store(gpu, grad_dtype, seed=1)
    P = len(flat.params)
    ps = list(flat.params)
    two_d = [i for i, p in enumerate(ps) if p.dim() > 1]
    zero_w, zero_g, nan_g = two_d[0], two_d[1], two_d[2]
    with torch.no_grad():
        ps[zero_w].zero_()
        ps[zero_g].main_grad.zero_()
        if max_norm is None:  # (with clipping a NaN gradient makes the global norm, so every ratio's input, NaN)
            ps[nan_g].main_grad.view(-1)[0] = float("nan")
    res = torch.zeros(3, device=gpu) if max_norm is not None else None
    plan = LarsPlan(flat, result=res)
    plan.compute(HP["trust_coef"], HP["weight_decay"], HP["eps"], max_norm)
    sq = plan.sq.double().cpu().tolist()
    got = plan.trust_dev.double().cpu().tolist()
    coef = 1.0
    if max_norm is not None:
        total = sum(sq[P:])
        rg = sum(_ref_sq(flat)[1])
        assert abs(res[0].item() - total) <= U * total and abs(res[0].item() - rg) <= BOUND * rg
        assert abs(res[1].item() - math.sqrt(rg)) <= BOUND * math.sqrt(rg)
        want_c = min(1.0, f32(max_norm) / (math.sqrt(res[0].item()) + 1e-6))
        coef = res[2].item()
        assert want_c < 0.5, "the clip must be active"
        assert abs(coef - want_c) <= K_C * U * want_c, (coef, want_c)
    want = _want_trust(sq, plan.plain.cpu().tolist(), P, HP, coef)
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        exact_one = ps[i].dim() <= 1 or i in (zero_w, zero_g) or (i == nan_g and max_norm is None)
        if exact_one:
            assert a == 1.0, (i, a)
        else:
            assert a != 1.0 and abs(a - b) <= K_T * U * b, (i, a, b)
            worst = max(worst, abs(a - b) / (U * b))
    print(f"trust {grad_dtype} max_norm {max_norm}: worst error {worst:.2f} u (bound {K_T} u)")
    # exclude_1d=False: the 1-D parameters get ratios too
    plan2 = LarsPlan(flat, result=res, exclude_1d=False)
    plan2.compute(HP["trust_coef"], HP["weight_decay"], HP["eps"], max_norm)
    one_d = [i for i, p in enumerate(ps) if p.dim() <= 1]
    assert all(plan2.trust_dev[i].item() != 1.0 for i in one_d)


def _clone_store(flat, mom):
    return flat.master.clone(), mom.clone(), flat.shadow.clone()


@GD
@pytest.mark.parametrize("first", [False, True], ids=["later", "first"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_update_with_unit_trust_is_bitwise_sgd_flat(gpu, grad_dtype, first, nesterov):
    from ddpx.ops.elementwise import sgd_flat_
    from ddpx.ops.lars import LarsPlan
    _, flat, pad, mom = _store(gpu, grad_dtype, seed=2)
    p0, b0, s0 = _clone_store(flat, mom)
    plan = LarsPlan(flat)
    plan.trust_dev.fill_(1.0)
    clip = torch.tensor(0.37, device=gpu)
    lr = torch.tensor(0.4, device=gpu)
    for use_clip in (False, True):
        flat.master.copy_(p0)
        flat.shadow.copy_(s0)
        mine = b0.clone()
        plan.update(0, flat.total, lr if use_clip else 0.4, 0.9, 5e-4, nesterov=nesterov, first=first,
                    clip=clip if use_clip else None, momentum_buf=mine)
        _still_nan(pad, flat.master, mine, flat.shadow, flat.grad)
        for i in range(len(flat.params)):
            sl = flat.slice(i)
            p, b, s = p0[sl].clone(), b0[sl].clone(), s0[sl].clone()
            sgd_flat_(p, b, flat.grad[sl], s, lr if use_clip else 0.4, 0.9, 5e-4, nesterov=nesterov, first=first,
                      clip=clip if use_clip else None)
            assert torch.equal(flat.master[sl], p) and torch.equal(mine[sl], b), (i, use_clip)
            assert torch.equal(flat.shadow[sl], s) and torch.equal(s, p.to(torch.bfloat16)), (i, use_clip)
            assert not torch.equal(p, p0[sl])


@GD
@pytest.mark.parametrize("max_norm", [None, 5.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_update_matches_fp64_given_the_device_trust_table(gpu, grad_dtype, max_norm, nesterov):
    """One launch from given fp32 w, g, momentum and the trust table the device computed (read back): every
    element within ``tests/_lars_ref.py``'s one-step bound with no error counted for the ratios themselves."""
    from ddpx.ops.lars import LarsPlan
    m, flat, pad, mom = _store(gpu, grad_dtype, seed=3)
    params = list(flat.params)
    res = torch.zeros(3, device=gpu) if max_norm is not None else None
    plan = LarsPlan(flat, result=res)
    plan.compute(HP["trust_coef"], HP["weight_decay"], HP["eps"], max_norm)
    trust = plan.trust_dev.double().cpu().tolist()
    assert sum(t != 1.0 for t in trust) >= 4
    ref = LarsFp64(params, nesterov=nesterov, max_grad_norm=max_norm, **HP)
    ref.B = [mom[flat.slice(i)].double().cpu().view(p.shape) for i, p in enumerate(params)]
    ref.step([p.main_grad for p in params], trust=trust)
    plan.update(0, flat.total, HP["lr"], HP["momentum"], HP["weight_decay"], nesterov=nesterov,
                clip=plan.coef_dev, momentum_buf=mom)
    worst = [0.0, 0.0]
    for i, p in enumerate(params):
        worst = [max(a, b) for a, b in zip(worst, ref.check(i, p, mom[flat.slice(i)], "one launch"))]
        assert torch.equal(flat.shadow[flat.slice(i)], flat.master[flat.slice(i)].to(torch.bfloat16))
    print(f"one launch {grad_dtype} max_norm {max_norm} nesterov {nesterov}: achieved fraction of the bound: "
          f"param {worst[0]:.3f} momentum {worst[1]:.3f}")
    _still_nan(pad, flat.master, mom, flat.shadow, flat.grad)


@GD
def test_sub_range_update_and_refused_arguments(gpu, grad_dtype):
    from ddpx.ops.lars import LarsPlan
    from ddpx.runtime import native
    _, flat, pad, mom = _store(gpu, grad_dtype, seed=4)
    p0, b0, s0 = _clone_store(flat, mom)
    g0 = flat.grad.clone()
    plan = LarsPlan(flat)
    plan.compute(HP["trust_coef"], HP["weight_decay"], HP["eps"])
    lo, hi = flat.offsets[3], flat.offsets[8]  # parameters 3 .. 7
    plan.update(lo, hi, 0.4, 0.9, 5e-4, momentum_buf=mom)
    bits = lambda t: t.view(torch.int32 if t.element_size() == 4 else torch.int16)  # noqa: E731
    inside = torch.zeros(flat.total, dtype=torch.bool, device=gpu)
    inside[lo:hi] = True
    for new, old in ((flat.master, p0), (mom, b0), (flat.shadow, s0)):
        assert torch.equal(bits(new)[~inside], bits(old)[~inside]), "written outside the range"
        changed = bits(new) != bits(old)
        assert not changed[pad].any()
        if new is not flat.shadow:  # (an update below half a bf16 ulp leaves a shadow element as it was)
            assert changed[inside & ~pad].float().mean().item() > 0.999, "the range was not updated"
    assert torch.equal(flat.shadow[inside & ~pad], flat.master[inside & ~pad].to(torch.bfloat16))
    assert torch.equal(bits(flat.grad), bits(g0))
    # a range that cuts a chunk, a range outside the plan's, mismatched and misaligned buffers: errors, no launch
    snap = _clone_store(flat, mom)
    with pytest.raises(ValueError, match="cuts the chunk"):
        plan.update(flat.offsets[6] + 8, hi, 0.4, 0.9, 5e-4, momentum_buf=mom)
    half = LarsPlan(flat, [(0, flat.offsets[5])])
    with pytest.raises(ValueError, match="cover"):
        half.update(0, flat.total, 0.4, 0.9, 5e-4, momentum_buf=mom)
    with pytest.raises(ValueError, match="numel"):
        plan.update(lo, hi, 0.4, 0.9, 5e-4, momentum_buf=mom[:-64])
    with pytest.raises(ValueError, match="momentum"):
        plan.update(lo, hi, 0.4, 0.9, 5e-4, momentum_buf=None)
    lib = native.kernels()
    args = (int(grad_dtype == torch.bfloat16), flat.shadow.data_ptr(), plan.table.data_ptr(), plan.n_chunks,
            plan.trust_dev.data_ptr(), None, None, 0.4, 0.9, 5e-4, 1.0, None, 0, 0, native.stream_handle())
    assert lib.ddpx_sgd_flat_chunks(flat.master.data_ptr() + 4, mom.data_ptr(), flat.grad.data_ptr(), *args) != 0
    assert lib.ddpx_sgd_flat_chunks(flat.master.data_ptr(), mom.data_ptr() + 8, flat.grad.data_ptr(), *args) != 0
    assert lib.ddpx_sgd_flat_chunks(flat.master.data_ptr(), mom.data_ptr(), flat.grad.data_ptr() + 2, *args) != 0
    assert lib.ddpx_sgd_flat_chunks(flat.master.data_ptr(), None, flat.grad.data_ptr(), *args) != 0
    assert lib.ddpx_lars_sumsq(flat.master.data_ptr() + 4, flat.grad.data_ptr(), args[0], plan.table.data_ptr(),
                               plan.n_chunks, plan.partials_buf.data_ptr(), native.stream_handle()) != 0
    torch.cuda.synchronize()
    for new, old in zip(_clone_store(flat, mom), snap):
        assert torch.equal(bits(new), bits(old))


# ----------------------------------------------------------------------------------------------- the optimizer
def _torch_norm(params_with_grads, max_norm):
    """torch's clip_grad_norm_ value for these gradients."""
    twins = []
    for g in params_with_grads:
        q = torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float32))
        q.grad = g.detach().float().clone()
        twins.append(q)
    return torch.nn.utils.clip_grad_norm_(twins, max_norm).item()


@pytest.mark.parametrize("max_norm", [None, 0.05], ids=["noclip", "clip"])
def test_captured_step_replays_equal_eager_steps(gpu, max_norm):
    """The training step captured as the trainer captures it (``capturable=True``): 3 replays of ONE captured step
    == the eager steps bit for bit in weights, momentum, shadow and the trust table; the table and the norm are
    recomputed on the device by every replay."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import LARS
    from ddpx.runtime.graphs import try_capture
    torch.manual_seed(5)
    a, b = MLP(hidden=256), MLP(hidden=256)
    b.load_state_dict(a.state_dict())
    for mdl in (a, b):
        ddpx.prepare_model(mdl, gpu)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, trust_coef=0.02, max_grad_norm=max_norm)
    oa = LARS(a.parameters(), capturable=True, **hp)
    ob = LARS(b.parameters(), **hp)
    xs = [torch.rand(128, 3072, device=gpu).to(torch.bfloat16) for _ in range(4)]
    ts = [torch.randint(0, 10, (128,), device=gpu) for _ in range(4)]

    def body_of(model, opt):
        def body(x, y):
            opt.zero_grad()
            loss, _ = model.forward_loss(x, y)
            loss.backward()
            opt.step()
            return loss
        return body

    body_a, body_b = body_of(a, oa), body_of(b, ob)
    oa.sync_lr()
    body_a(xs[0], ts[0])  # the trainer's eager warm-up step
    graph, err = try_capture(body_a, xs[1], ts[1], a, oa)
    assert graph is not None, err
    ta, tb, na, nb = [], [], [], []
    for i in range(1, 4):
        graph(xs[i], ts[i])
        ta.append(oa.trust_ratio_dev.clone())
        if max_norm is not None:
            na.append(oa.grad_norm_dev.item())
    for i in range(4):
        body_b(xs[i], ts[i])
        tb.append(ob.trust_ratio_dev.clone())
        if max_norm is not None:
            nb.append(ob.grad_norm_dev.item())
            want = _torch_norm([p.main_grad for p in b.parameters()], max_norm)
            assert want > 2 * max_norm, "the clip must be active"
            assert abs(nb[-1] - want) <= BOUND * want, (i, nb[-1], want)
    torch.cuda.synchronize()
    for x, y in zip(ta, tb[1:]):
        assert torch.equal(x, y)
    assert not torch.equal(ta[0], ta[1]) and not torch.equal(ta[1], ta[2])  # recomputed per replay
    fa, fb = oa.flat, ob.flat
    weights = [fa.index[id(p)] for p in a.parameters() if p.dim() > 1]
    assert all(ta[-1][j].item() != 1.0 for j in weights) and sum(t.item() == 1.0 for t in ta[-1]) == 3  # 3 biases
    assert na == nb[1:]
    assert torch.equal(fa.master, fb.master) and torch.equal(oa.momentum_buffer, ob.momentum_buffer)
    assert torch.equal(fa.shadow, fb.shadow) and torch.equal(fa.shadow, fa.master.to(torch.bfloat16))
    assert fa.fused_opt is None and not oa.fused_active()


@pytest.fixture(scope="module")
def pg(gpu):
    import os
    import torch.distributed as dist
    from tests._dist_util import free_port
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("max_norm", [None, 0.05], ids=["noclip", "clip"])
def test_replicated_ddp_with_bucket_overlap_is_bitwise_the_plain_step(gpu, pg, max_norm):
    """World size 1, replicated plan, per-bucket optimizer overlap: partials bucket by bucket, then the updates.
    Buckets end at parameter boundaries, so the chunk tables, hence all bits, are the single-process step's."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import LARS
    from ddpx.parallel.comm import RcclComm
    from ddpx.parallel.ddp import DistributedDataParallel
    torch.manual_seed(0)
    a, b = MLP(hidden=512), MLP(hidden=512)
    b.load_state_dict(a.state_dict())
    ddpx.prepare_model(a, gpu)
    ddpx.prepare_model(b, gpu)
    comm = RcclComm(gpu)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, trust_coef=0.02, max_grad_norm=max_norm)
    oa = LARS(a.parameters(), **hp)
    da = DistributedDataParallel(a, comm=comm, bucket_cap_mb=1.0, first_bucket_mb=0.25, reduce_single=True,
                                 overlap_optimizer=True)
    assert len(da.bucket_ranges) >= 2
    da.attach_optimizer(oa)
    ob = LARS(b.parameters(), **hp)
    x = torch.rand(256, 3072, device=gpu).to(torch.bfloat16)
    t = torch.randint(0, 10, (256,), device=gpu)
    for _ in range(3):
        for net, opt in ((da, oa), (b, ob)):
            opt.zero_grad()
            loss, _ = net.forward_loss(x, t)
            loss.backward()
            opt.step()
    torch.cuda.synchronize()
    assert len(oa._norm_plan.ranges) == len(da.bucket_ranges)  # the per-bucket path ran
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    fa, fb = oa.flat, ob.flat
    for p, q in zip(a.parameters(), b.parameters()):
        assert oa.trust_ratio_dev[fa.index[id(p)]] == ob.trust_ratio_dev[fb.index[id(q)]]
    da.close()
    comm.close()


def _twin_lars_step(params, bufs, hp):
    """The reference LARS in plain fp32 torch ops, parameter by parameter."""
    with torch.no_grad():
        for p, buf in zip(params, bufs):
            g = p.grad
            wn, gn = p.norm(), g.norm()
            t = 1.0
            if p.dim() > 1 and wn > 0 and gn > 0:
                t = hp["trust_coef"] * wn / (gn + hp["weight_decay"] * wn + hp["eps"])
            d = (g + hp["weight_decay"] * p) * t
            buf.mul_(hp["momentum"]).add_(d)
            p.sub_(hp["lr"] * buf)


def test_whole_model_tracks_a_torch_fp32_twin(gpu):
    """``--model mlp --hidden 256 --batch_size 128 --dtype bf16 --optimizer lars`` built as the training scripts
    build it, 6 steps on one batch against a torch fp32 twin that runs the reference LARS from the same init, within
    the tolerance ``smoke()`` uses for its SGD twin (3 % + 0.02 on every loss), as the AdamW whole-model test."""
    from ddpx.models import MLP
    from ddpx.optim import LARS
    from ddpx.train.app import build_model_and_optimizer, build_parser
    torch.manual_seed(0)
    args = build_parser("t").parse_args(["1", "1", "--model", "mlp", "--hidden", "256", "--batch_size", "128",
                                         "--dtype", "bf16", "--kernels", "native", "--optimizer", "lars"])
    model, opt = build_model_and_optimizer(args, gpu)
    assert type(opt) is LARS and model.use_native and opt.flat.fused_opt is None and not opt.fused_active()
    twin = MLP(hidden=256, layers=3)
    twin.load_state_dict(model.state_dict())
    twin = twin.to(gpu)
    twin.use_native = False
    twin.compute_dtype = torch.float32
    g = opt.param_groups[0]
    hp = {k: g[k] for k in ("lr", "momentum", "weight_decay", "trust_coef", "eps")}
    tparams = list(twin.parameters())
    bufs = [torch.zeros_like(p) for p in tparams]
    w0 = [p.detach().clone() for p in model.parameters()]
    x = torch.rand(128, 3072, device=gpu).to(torch.bfloat16)
    y = torch.randint(0, 10, (128,), device=gpu)
    losses, ref = [], []
    for _ in range(6):
        opt.zero_grad()
        loss, _ = model.forward_loss(x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        for p in tparams:
            p.grad = None
        tl = torch.nn.functional.cross_entropy(twin(x.float()), y)
        tl.backward()
        _twin_lars_step(tparams, bufs, hp)
        ref.append(float(tl.item()))
    print("lars losses", losses, "torch fp32 twin", ref)
    assert all(math.isfinite(v) for v in losses), losses
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 0.03 * abs(b) + 0.02, (losses, ref)
    f = opt.flat
    for p, p0 in zip(model.parameters(), w0):
        assert not torch.equal(p.detach(), p0)
        assert (opt.trust_ratio_dev[f.index[id(p)]].item() == 1.0) == (p.dim() <= 1)
    assert opt.flat.fused_opt is None and opt.step_count == 6


def test_full_checkpoint_round_trip(gpu, tmp_path):
    """3 steps, save, continue in a fresh model + optimizer loaded from the file: the next 2 steps are bitwise the
    uninterrupted run's (weights, momentum, shadow, trust table)."""
    from ddpx.optim import SGD, LARS
    from ddpx.runtime.flat_params import FlatParams
    from ddpx.train.checkpoint import load_full_checkpoint, save_full_checkpoint
    path = str(tmp_path / "full.pt")

    def make(seed):
        torch.manual_seed(seed)
        m = _Odd(_shapes()).to(gpu)
        return m, FlatParams(m, shadow_dtype=torch.bfloat16)

    m, flat = make(13)
    opt = LARS(m.parameters(), max_grad_norm=5.0, **HP)
    for step in range(5):
        if step == 3:
            save_full_checkpoint(path, m, opt, None, epoch=0)
        opt.zero_grad()
        _fill(flat, 40 + step)
        opt.step()
    m2, flat2 = make(99)  # another init: everything must come from the file
    opt2 = LARS(m2.parameters(), lr=0.5, momentum=0.5, weight_decay=0.5, trust_coef=0.5, eps=1.0, max_grad_norm=5.0)
    assert load_full_checkpoint(path, m2, opt2, None, map_location=gpu) == 1
    assert opt2.step_count == 3 and opt2.param_groups[0]["trust_coef"] == HP["trust_coef"]
    for step in (3, 4):
        opt2.zero_grad()
        _fill(flat2, 40 + step)
        opt2.step()
    for i in range(len(flat.params)):
        sl = flat.slice(i)
        for a, b in ((flat.master, flat2.master), (flat.shadow, flat2.shadow),
                     (opt.momentum_buffer, opt2.momentum_buffer)):
            assert torch.equal(a[sl], b[sl]), i
    assert torch.equal(opt.trust_ratio_dev, opt2.trust_ratio_dev)
    assert torch.equal(opt.grad_norm_dev, opt2.grad_norm_dev)
    # the other optimizer's file is refused
    m3, _ = make(1)
    with pytest.raises(ValueError, match="another optimizer"):
        load_full_checkpoint(path, m3, SGD(m3.parameters(), lr=0.1, momentum=0.9), None, map_location=gpu)
