"""Gradient clipping by global norm on the GPU: the flat sum-of-squares kernels, the clip factor folded into
the flat SGD kernel, ``SGD(max_grad_norm=...)``, HIP-graph capture and the functional ``clip_grad_norm_``.

Tolerance of the sum of squares (``BOUND``), from the kernel's own summation shape
(``csrc/kernels/grad_norm.hip``).  All summands are squares (>= 0), so a sum in which every summand passes
through at most ``d`` fp32 roundings has a relative error of at most ``d * 2^-24`` to first order (each rounding
multiplies a partial sum by (1 + e), |e| <= 2^-24, and nothing cancels).  The roundings on the longest path:

* 33  one accumulator's fma chain: a chunk of CHUNK = 32768 elements is CHUNK / 16 B-vector-width vectors,
      dealt to 256 threads x 4 accumulators = 32 elements per accumulator for fp32 (8 vectors of 4) and for
      bf16 (4 vectors of 8); the square is exact inside the fma; + 1 for the scalar tail on accumulator 0;
* 2   (a0 + a1) + (a2 + a3);
* 6   the 64-lane butterfly;
* 2   (w0 + w1) + (w2 + w3) over the 4 waves through LDS;
* 1   the fp64 total (its own error is ~2^-53 per add: nothing at this scale) rounded to the fp32 scalar.

44 roundings -> 44 * 2^-24 = 2.6e-6.  The norm is sqrt(sq): half the relative error of sq plus one rounding,
which the same bound covers.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TERMS = 33 + 2 + 6 + 2 + 1
BOUND = TERMS * 2.0 ** -24


class _Odd(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n) * 0.1) for n in sizes])


def _sizes():
    from ddpx.ops.clip import CHUNK
    return [1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 5, 2 * CHUNK + 1]


def _store(gpu, grad_dtype, seed=0):
    """A flat store over the odd-sized parameters with random gradients and NaN in every padding element."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m = _Odd(_sizes()).to(gpu)
    flat = FlatParams(m, grad_dtype=grad_dtype)
    _fill(flat, seed)
    return m, flat


def _fill(flat, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat.grad.fill_(float("nan"))
    for p in flat.params:
        p.main_grad.copy_(torch.randn(p.shape, generator=g).to(flat.device))
        flat.grad_done(p)


def _ref_sq(flat, lo=0, hi=None):
    """fp64 sum of squares over the parameter views, restricted to flat [lo, hi)."""
    hi = flat.total if hi is None else hi
    s = 0.0
    for o, n in zip(flat.offsets, flat.numels):
        a, b = max(o, lo), min(o + n, hi)
        if a < b:
            s += flat.grad[a:b].double().square().sum().item()
    return s


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_sumsq_matches_fp64_and_never_reads_padding(gpu, grad_dtype):
    from ddpx.ops.clip import GradNormPlan
    _, flat = _store(gpu, grad_dtype)
    assert torch.isnan(flat.grad.float()).any(), "the store has padding and it is NaN"
    plan = GradNormPlan(flat)
    plan.compute(1.0)
    ref = _ref_sq(flat)
    sq = plan.sq.item()
    print(f"sumsq {grad_dtype}: got {sq!r} ref {ref!r} rel {abs(sq - ref) / ref:.3e} bound {BOUND:.3e}")
    assert math.isfinite(sq) and abs(sq - ref) <= BOUND * ref
    assert abs(plan.norm_dev.item() - math.sqrt(ref)) <= BOUND * math.sqrt(ref)
    # per-chunk partials against fp64, chunk by chunk (a wrong chunk cannot hide in the total)
    parts = plan.partials_buf.cpu().tolist()
    for (s, n), got in zip(plan.chunks, parts):
        want = flat.grad[s:s + n].double().square().sum().item()
        assert abs(got - want) <= BOUND * want, (s, n, got, want)
    # a shard: ranges that cut the biggest parameter in the middle, at a 64-element boundary
    big = max(range(len(flat.numels)), key=lambda i: flat.numels[i])
    cut = flat.offsets[big] + 64 * 517
    halves = []
    for (lo, hi) in ((0, cut), (cut, flat.total)):
        pl = GradNormPlan(flat, [(lo, hi)])
        pl.compute(1.0)
        want = _ref_sq(flat, lo, hi)
        assert abs(pl.sq.item() - want) <= BOUND * want, (lo, hi)
        halves.append(pl.sq.item())
    assert abs(halves[0] + halves[1] - ref) <= BOUND * ref


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_sumsq_is_bitwise_reproducible_and_independent_of_the_split(gpu, grad_dtype):
    from ddpx.ops.clip import GradNormPlan
    _, flat = _store(gpu, grad_dtype, seed=1)
    plan = GradNormPlan(flat)
    plan.compute(0.5)
    p1, r1 = plan.partials_buf.clone(), plan._res.clone()
    plan.partials_buf.zero_()
    plan.compute(0.5)
    assert torch.equal(plan.partials_buf, p1) and torch.equal(plan._res, r1)
    big = max(range(len(flat.numels)), key=lambda i: flat.numels[i])
    c1, c2 = sorted((flat.offsets[3] + 64, flat.offsets[big] + 64 * 100))  # both inside a parameter
    split = GradNormPlan(flat, [(0, c1), (c1, c2), (c2, flat.total)])
    for k in range(3):
        split.partials(k)
        split.reduce(accumulate=k > 0, span=(k, k + 1))
    a, b = split.sq.item(), plan.sq.item()
    assert abs(a - b) <= BOUND * b, (a, b)


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_sgd_flat_clip_factor_one_is_bitwise_sgd_flat(gpu, grad_dtype, shadow):
    from ddpx.ops.elementwise import sgd_flat_
    torch.manual_seed(2)
    n = 4099  # vector body + scalar tail
    one = torch.ones((), device=gpu)
    p0 = torch.randn(n, device=gpu)
    out = []
    for clip in (None, one):
        p, buf = p0.clone(), torch.zeros(n, device=gpu)
        sh = torch.zeros(n, dtype=torch.bfloat16, device=gpu) if shadow else None
        gen = torch.Generator(device="cpu").manual_seed(3)
        for _ in range(2):
            g = torch.randn(n, generator=gen).to(gpu).to(grad_dtype)
            sgd_flat_(p, buf, g, sh, 0.4, 0.9, 5e-4, clip=clip)
        out.append((p, buf, sh))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    if shadow:
        assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[1][2], out[1][0].to(torch.bfloat16))
    assert not torch.equal(out[0][0], p0)


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
def test_three_clipped_steps_match_torch(gpu, max_norm):
    from ddpx.optim.sgd import SGD
    m, flat = _store(gpu, torch.float32, seed=4)
    twin = _Odd(_sizes()).to(gpu)
    twin.load_state_dict(m.state_dict())
    opt = SGD(m.parameters(), lr=0.4, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
    topt = torch.optim.SGD(twin.parameters(), lr=0.4, momentum=0.9, weight_decay=5e-4)
    for step in range(3):
        opt.zero_grad()
        _fill(flat, 10 + step)
        for p, q in zip(m.parameters(), twin.parameters()):
            q.grad = p.main_grad.detach().clone()
        opt.step()
        tn = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
        topt.step()
        got, want = opt.grad_norm_dev.item(), tn.item()
        print(f"step {step}: norm {got!r} torch {want!r} coef {opt.clip_coef_dev.item()!r}")
        assert (want > 100 * max_norm) if max_norm < 1 else (want < max_norm / 100)
        assert abs(got - want) <= BOUND * want
        assert opt.clip_coef_dev.item() == 1.0 if max_norm > 1 else opt.clip_coef_dev.item() < 0.01
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6)  # as test_sgd_flat_matches_torch


def test_max_grad_norm_turns_the_fused_optimizer_off(gpu):
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim.sgd import SGD
    a, b = MLP(hidden=256), MLP(hidden=256)
    ddpx.prepare_model(a, gpu)
    ddpx.prepare_model(b, gpu)
    assert SGD(a.parameters(), lr=0.1, fused_backward=True).fused_active() is True
    o = SGD(b.parameters(), lr=0.1, fused_backward=True, max_grad_norm=1.0)
    assert o.fused_active() is False and b.fc0.weight._ddpx_flat.fused_opt is None


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_native_mlp_clipped_steps_match_torch_twin(gpu, grad_dtype):
    """Hidden 256, batch 128, 3 clipped steps: the native path vs fp32 torch math with bf16 rounding at the native
    path's storage points (``_mlp_reference``), ``clip_grad_norm_`` and ``torch.optim.SGD``, with
    ``test_mlp_native_matches_reference``'s tolerances (2e-3 fp32, 1e-2 bf16 gradients; loss 1e-3).

    Those tolerances are for a gradient taken at the SAME weights, so the twin starts every step from the native
    model's weights and momentum and each step's loss, pre-clip norm and update are compared.  A twin left on its
    own trajectory measures something else: with bf16 gradient buffers the 1.7e-3 rounding of step 1's gradient
    moves the weights enough to flip bf16 roundings and ReLU decisions of later activations, and the gradients at
    the two weight sets then differ by 1.2e-2 (step 2) and 3e-2 (step 3) while the kernels' error at equal weights
    stays 1.7e-3; measured, the 3-step update of fc0.weight differed by 1.14e-2 with clipping and by 1.62e-2
    with no clipping at all (fp32 gradients: 1e-4 either way)."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim.sgd import SGD
    from tests.test_gpu_kernels import _mlp_reference, _rel
    torch.manual_seed(4)
    max_norm = 0.05
    m = MLP(hidden=256, layers=3)
    ddpx.prepare_model(m, gpu, grad_dtype=grad_dtype)
    flat = m.fc0.weight._ddpx_flat
    named = list(m.named_parameters())
    tw = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named}
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
    topt = torch.optim.SGD([tw[n] for n, _ in named], lr=0.05, momentum=0.9, weight_decay=5e-4)
    tol = 2e-3 if grad_dtype == torch.float32 else 1e-2
    for step in range(3):
        x = torch.rand(128, 3072, device=gpu).to(torch.bfloat16)
        t = torch.randint(0, 10, (128,), device=gpu)
        before = {}
        with torch.no_grad():
            for n, p in named:  # the twin takes over the native model's state
                before[n] = p.detach().clone()
                tw[n].copy_(p)
                if step:
                    buf = opt.momentum_buffer[flat.slice(flat.index[id(p)])].view(p.shape)
                    topt.state[tw[n]]["momentum_buffer"] = buf.clone()
        opt.zero_grad()
        loss, _ = m.forward_loss(x, t)
        loss.backward()
        opt.step()
        W = [_bf(tw[f"fc{i}.weight"].detach()) for i in range(3)]
        b = [tw[f"fc{i}.bias"].detach() for i in range(3)]
        rl, rg = _mlp_reference(x, t, W, b)
        for n, _ in named:
            tw[n].grad = rg[n].clone()
        tn = torch.nn.utils.clip_grad_norm_([tw[n] for n, _ in named], max_norm)
        topt.step()
        rels = {n: _rel(p.detach() - before[n], tw[n].detach() - before[n]) for n, p in named}
        print(f"step {step}: loss {loss.item():.6f} ref {rl.item():.6f} norm {opt.grad_norm_dev.item():.6f} "
              f"torch {tn.item():.6f} update rel {max(rels.values()):.2e}")
        assert tn.item() > 2 * max_norm, "the clip must be active"
        assert abs(loss.item() - rl.item()) < 1e-3
        assert abs(opt.grad_norm_dev.item() - tn.item()) <= tol * tn.item()
        for n, r in rels.items():
            assert r < tol, (step, n, r)


def test_clipped_step_in_a_hip_graph(gpu):
    """The clipped training step captured as the trainer captures it: 3 replays == 3 eager steps bit for bit, and
    the norm is recomputed on the device by every replay."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim.sgd import SGD
    from ddpx.runtime.graphs import try_capture
    torch.manual_seed(5)
    a, b = MLP(hidden=256), MLP(hidden=256)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        ddpx.prepare_model(m, gpu)
    oa = SGD(a.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, max_grad_norm=0.05)
    ob = SGD(b.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=0.05)
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
    na, nb = [], []
    for i in range(1, 4):
        graph(xs[i], ts[i])
        na.append(oa.grad_norm_dev.item())
    for i in range(4):
        body_b(xs[i], ts[i])
        nb.append(ob.grad_norm_dev.item())
    torch.cuda.synchronize()
    assert na == nb[1:], (na, nb)
    assert len(set(na)) == 3, na  # recomputed per replay, not baked in at capture
    assert all(v > 0.1 for v in na), na  # the clip is active
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(oa.momentum_buffer, ob.momentum_buffer)


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
def test_functional_clip_grad_norm(gpu, grad_dtype):
    from ddpx.optim import clip_grad_norm_
    m, flat = _store(gpu, grad_dtype, seed=6)
    before = [p.main_grad.detach().clone() for p in flat.params]
    ref = math.sqrt(_ref_sq(flat))
    norm = clip_grad_norm_(m, 2.0)
    assert norm.is_cuda and norm.dtype == torch.float32
    got = norm.item()
    assert math.isfinite(got) and abs(got - ref) <= BOUND * ref
    coef = flat._clip_plan.coef_dev
    assert abs(coef.item() - 2.0 / (ref + 1e-6)) <= 4 * BOUND * coef.item()
    for p, g0 in zip(flat.params, before):
        assert torch.equal(p.main_grad, (g0.float() * coef).to(grad_dtype))
    # below the threshold nothing changes
    after = [p.main_grad.detach().clone() for p in flat.params]
    clip_grad_norm_(m.parameters(), 1e9)
    assert flat._clip_plan.coef_dev.item() == 1.0
    for p, g0 in zip(flat.params, after):
        assert torch.equal(p.main_grad, g0)
