"""LAMB on the GPU: ``ddpx_lamb_moments`` (moments and per-chunk partial sums), the trust table, ``ddpx_lamb_apply``
against fp64, ``ddpx.optim.LAMB`` eager against captured, under replicated DDP, with a skipped parameter, on a
whole model and through a full checkpoint.

Tolerances, all counted from the kernels' rounding sequences (``csrc/kernels/lamb.hip``); u = 2^-24.

* m and v after one launch: AdamW's per-step bounds (``tests/test_gpu_adamw.py``): |m' - m^| <= K_M u (|m| + |g|),
  |v' - v^| <= K_V u v^, with + 1 and + 2 when a gradient scale is applied (the scaled g carries its own rounding).
* Partial sums: ``tests/_lars_ref.py``'s ``SUMSQ`` (44 u) against the fp64 sum of the squares of the fp32 terms the
  kernel squares.  For w^2 the terms are the weights.  For u^2 they are ``lamb_u`` of the m and v the device wrote
  (read back), evaluated on the host in the kernel's own fp32 sequence (IEEE division, square root and add are
  correctly rounded on both sides; the one fma is taken through fp64, where its product is exact): the bound is
  about the summation, so the reference sums in fp64 what the kernel sums in fp32.  A total completed by a second,
  accumulating reduction is rounded twice: + u.
* Trust ratio from the fp32 totals the kernel read: ``K_T`` = 3 u (two square roots and the division).
* The apply pass, one launch given the device's m, v and table, and several steps: ``tests/_lamb_ref.py``.
"""
import math

import pytest
import torch

from tests._lamb_ref import K_M, K_T, K_V, LambFp64
from tests._lars_ref import SUMSQ, TINY, U, f32
from tests.test_gpu_lars import _fill, _Odd, _pad_mask, _shapes, _still_nan

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
MOM = dict(betas=HP["betas"], eps=HP["eps"], weight_decay=HP["weight_decay"])
GD = pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bc(gpu, t, betas=HP["betas"]):
    """The device's bias corrections of step t (``ddpx_adamw_advance`` from a counter at t - 1)."""
    from ddpx.ops.elementwise import adamw_advance_
    counter = torch.tensor([t - 1], dtype=torch.int32, device=gpu)
    bc = torch.ones(2, dtype=torch.float32, device=gpu)
    adamw_advance_(counter, bc, *betas)
    assert counter.item() == t
    return bc


def _store(gpu, grad_dtype, seed=0):
    """The odd-shaped store of ``tests/test_gpu_lars.py`` with random gradients, m and v >= 0, and NaN in every
    padding element of master, gradient, both states and the shadow."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    mdl = _Odd(_shapes()).to(gpu)
    flat = FlatParams(mdl, grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)
    pad = _pad_mask(flat)
    assert pad.any()
    m = torch.randn(flat.total, device=gpu) * 0.05
    v = (torch.randn(flat.total, device=gpu) * 0.1).square()
    nan = float("nan")
    for t in (flat.master, flat.shadow, m, v):
        t[pad] = nan
    _fill(flat, seed)
    return mdl, flat, pad, m, v


def _u_as_the_kernel(w, m, v, bc, eps, wd):
    """``lamb_u`` in the kernel's fp32 sequence, on the host, from fp32 CPU tensors."""
    bc1, bc2s = bc[0].cpu(), bc[1].cpu()
    e, d = torch.tensor(eps, dtype=torch.float32), torch.tensor(wd, dtype=torch.float32)
    r = (m / bc1) / (v.sqrt() / bc2s + e)
    return (d.double() * w.double() + r.double()).float()


def _check_moments(flat, plan, w0, m0, v0, m1, v1, bc, scale, label):
    """m', v' against fp64 within AdamW's bounds and every chunk's two partials within SUMSQ; returns the worst
    achieved fractions (m, v, sum w^2, sum u^2)."""
    b1, b2 = HP["betas"]
    w1, fb2, w2 = f32(1.0 - b1), f32(b2), f32(1.0 - b2)
    km, kv = K_M + (1 if scale is not None else 0), K_V + (2 if scale is not None else 0)
    g = flat.grad.float().double().cpu() * (f32(scale) if scale is not None else 1.0)
    m0d, v0d = m0.double().cpu(), v0.double().cpu()
    mref = m0d + (g - m0d) * w1
    vref = fb2 * v0d + w2 * g * g
    wc, m1c, v1c = w0.cpu(), m1.cpu(), v1.cpu()
    uk = _u_as_the_kernel(wc, m1c, v1c, bc, f32(HP["eps"]), f32(HP["weight_decay"])).double()
    part = plan.partials_buf.double().cpu()
    worst = [0.0] * 4
    for j, (s, n, pid) in enumerate(plan.chunks):
        assert flat.offsets[pid] <= s and s + n <= flat.offsets[pid] + flat.numels[pid]
        sl = slice(s, s + n)
        fm = ((m1c[sl].double() - mref[sl]).abs() / (km * U * (m0d[sl].abs() + g[sl].abs()) + TINY)).max().item()
        fv = ((v1c[sl].double() - vref[sl]).abs() / (kv * U * vref[sl] + TINY)).max().item()
        sw, su = wc[sl].double().square().sum().item(), uk[sl].square().sum().item()
        fw = abs(part[j, 0].item() - sw) / (SUMSQ * sw)
        fu = abs(part[j, 1].item() - su) / (SUMSQ * su)
        got = [fm, fv, fw, fu]
        assert all(math.isfinite(x) and x <= 1.0 for x in got), (label, j, (s, n, pid), got)
        worst = [max(a, b) for a, b in zip(worst, got)]
    return worst


@GD
def test_moments_kernel(gpu, grad_dtype):
    from ddpx.ops.lamb import LambPlan
    _, flat, pad, m, v = _store(gpu, grad_dtype)
    P = len(flat.params)
    w0, m0, v0, s0, g0 = flat.master.clone(), m.clone(), v.clone(), flat.shadow.clone(), flat.grad.clone()
    bc = _bc(gpu, 3)
    plan = LambPlan(flat)
    clip = torch.tensor(0.37, device=gpu)
    for scale in (None, 0.37):
        m.copy_(m0)
        v.copy_(v0)
        plan.partials_buf.fill_(float("nan"))
        plan.moments(0, m, v, bc, clip=clip if scale is not None else None, **MOM)
        plan.reduce()
        part1, sq1, m1, v1 = plan.partials_buf.clone(), plan.sq.clone(), m.clone(), v.clone()
        assert torch.isfinite(part1).all() and torch.isfinite(sq1).all(), "NaN padding leaked into a sum"
        _still_nan(pad, m, v, flat.master, flat.shadow, flat.grad)
        assert torch.equal(_bits(flat.master), _bits(w0)) and torch.equal(_bits(flat.shadow), _bits(s0))
        assert torch.equal(_bits(flat.grad), _bits(g0))
        assert not torch.equal(m1[~pad], m0[~pad]) and not torch.equal(v1[~pad], v0[~pad])
        worst = _check_moments(flat, plan, w0, m0, v0, m1, v1, bc, scale, f"{grad_dtype} scale {scale}")
        print(f"moments {grad_dtype} scale {scale}: achieved fraction of the bound: m {worst[0]:.3f} v {worst[1]:.3f} "
              f"sum w^2 {worst[2]:.3f} sum u^2 {worst[3]:.3f}")
        # a second run from restored inputs: the same bits
        m.copy_(m0)
        v.copy_(v0)
        plan.partials_buf.zero_()
        plan.sq.zero_()
        plan.moments(0, m, v, bc, clip=clip if scale is not None else None, **MOM)
        plan.reduce()
        for a, b in ((m, m1), (v, v1), (plan.partials_buf, part1), (plan.sq, sq1)):
            assert torch.equal(_bits(a), _bits(b))
    # (the loop's last run: scale 0.37) two shards that cut the biggest parameter at a 64-element boundary, the
    # second accumulated onto the first
    big = max(range(P), key=lambda i: flat.numels[i])
    cut = flat.offsets[big] + 64 * 517
    sq = torch.zeros(2 * P, device=gpu)
    split = LambPlan(flat, [(0, cut), (cut, flat.total)], sq=sq)
    m.copy_(m0)
    v.copy_(v0)
    split.moments(1, m, v, bc, clip=clip, **MOM)
    split.moments(0, m, v, bc, clip=clip, **MOM)
    assert torch.equal(_bits(m), _bits(m1)) and torch.equal(_bits(v), _bits(v1))  # element-wise: the same bits
    split.reduce(span=(0, 1))
    after = [i for i in range(P) if flat.offsets[i] >= cut]
    assert after and all(sq[i].item() == 0 and sq[P + i].item() == 0 for i in after)
    split.reduce(accumulate=True, span=(1, 2))
    wc = w0.cpu()
    uk = _u_as_the_kernel(wc, m1.cpu(), v1.cpu(), bc, f32(HP["eps"]), f32(HP["weight_decay"])).double()
    for i in range(P):
        sl = flat.slice(i)
        for got, want in ((sq[i].item(), wc[sl].double().square().sum().item()),
                          (sq[P + i].item(), uk[sl].square().sum().item())):
            assert abs(got - want) <= (SUMSQ + U) * want, (i, got, want)
        if i != big:  # one piece: the same chunks, the same bits
            assert sq[i] == sq1[i] and sq[P + i] == sq1[P + i]


@GD
def test_trust_table(gpu, grad_dtype):
    from ddpx.ops.lamb import LambPlan
    _, flat, pad, m, v = _store(gpu, grad_dtype, seed=1)
    P = len(flat.params)
    ps = list(flat.params)
    two_d = [i for i, p in enumerate(ps) if p.dim() > 1]
    one_d = [i for i, p in enumerate(ps) if p.dim() <= 1]
    zero_w, all_zero, nan_g = two_d[0], two_d[1], two_d[2]
    with torch.no_grad():
        ps[zero_w].zero_()
        ps[all_zero].zero_()
        ps[all_zero].main_grad.zero_()
        m[flat.slice(all_zero)] = 0
        v[flat.slice(all_zero)] = 0
    m0, v0 = m.clone(), v.clone()
    bc = _bc(gpu, 2)
    plan = LambPlan(flat)

    def run(pl):
        m.copy_(m0)
        v.copy_(v0)
        pl.compute(m, v, bc, **MOM)
        sq = pl.sq.double().cpu().tolist()
        return sq, pl.trust_dev.double().cpu().tolist()

    def check(sq, got, ones):
        worst, moved = 0.0, 0
        for i, a in enumerate(got):
            if ps[i].dim() <= 1 or i in ones:
                assert a == 1.0, (i, a)
                continue
            want = math.sqrt(sq[i]) / math.sqrt(sq[P + i])
            assert a != 1.0 and abs(a - want) <= K_T * U * want, (i, a, want)
            worst = max(worst, abs(a - want) / (K_T * U * want))
            moved += 1
        return worst, moved

    sq, got = run(plan)
    assert sq[zero_w] == 0 and sq[P + zero_w] > 0 and sq[all_zero] == 0 and sq[P + all_zero] == 0
    worst, moved = check(sq, got, (zero_w, all_zero))
    assert moved >= 4
    print(f"trust {grad_dtype}: achieved fraction of the bound {worst:.3f} ({moved} ratios != 1)")
    # a NaN gradient: its m, v, u and u^2 total are NaN, its ratio reads 1, nobody else's changes
    with torch.no_grad():
        ps[nan_g].main_grad.view(-1)[0] = float("nan")
    sq2, got2 = run(plan)
    assert math.isnan(sq2[P + nan_g]) and all(math.isfinite(x) for i, x in enumerate(sq2) if i != P + nan_g)
    check(sq2, got2, (zero_w, all_zero, nan_g))
    assert all(a == b for i, (a, b) in enumerate(zip(got, got2)) if i != nan_g)
    # exclude_1d=False: the 1-D parameters get ratios too
    plan2 = LambPlan(flat, exclude_1d=False)
    _, got3 = run(plan2)
    assert all(got3[i] != 1.0 for i in one_d)


@GD
def test_apply_matches_fp64_given_the_device_moments_and_trust_table(gpu, grad_dtype):
    """One apply launch from given fp32 w and the m, v and trust table the device computed (read back): every
    element within ``tests/_lamb_ref.py``'s one-launch bound, no error counted for m, v and the ratios."""
    from ddpx.ops.lamb import LambPlan
    _, flat, pad, m, v = _store(gpu, grad_dtype, seed=3)
    params = list(flat.params)
    bc = _bc(gpu, 3)
    plan = LambPlan(flat)
    plan.compute(m, v, bc, **MOM)
    trust = plan.trust_dev.double().cpu().tolist()
    assert sum(t != 1.0 for t in trust) >= 4
    m1, v1, g0 = m.clone(), v.clone(), flat.grad.clone()
    ref = LambFp64(params, **HP)
    ref.step([p.main_grad for p in params], trust=trust, bc=bc.cpu().tolist(),
             moments=([m[flat.slice(i)] for i in range(len(params))], [v[flat.slice(i)] for i in range(len(params))]))
    lr = torch.tensor(HP["lr"], device=gpu)
    plan.apply(0, flat.total, lr, m, v, bc, HP["eps"], HP["weight_decay"])
    worst = 0.0
    for i, p in enumerate(params):
        worst = max(worst, ref.check(i, p, label="one launch")[0])
        assert torch.equal(flat.shadow[flat.slice(i)], flat.master[flat.slice(i)].to(torch.bfloat16))
    print(f"apply {grad_dtype}: achieved fraction of the one-launch bound {worst:.3f}")
    _still_nan(pad, flat.master, m, v, flat.shadow, flat.grad)
    assert torch.equal(_bits(m), _bits(m1)) and torch.equal(_bits(v), _bits(v1))
    assert torch.equal(_bits(flat.grad), _bits(g0))


@GD
def test_sub_range_apply_and_refused_arguments(gpu, grad_dtype):
    from ddpx.ops.lamb import LambPlan
    from ddpx.runtime import native
    _, flat, pad, m, v = _store(gpu, grad_dtype, seed=4)
    bc = _bc(gpu, 2)
    plan = LambPlan(flat)
    plan.compute(m, v, bc, **MOM)
    p0, s0, m1, v1, g0 = flat.master.clone(), flat.shadow.clone(), m.clone(), v.clone(), flat.grad.clone()
    lo, hi = flat.offsets[3], flat.offsets[8]  # parameters 3 .. 7
    plan.apply(lo, hi, HP["lr"], m, v, bc, HP["eps"], HP["weight_decay"])
    inside = torch.zeros(flat.total, dtype=torch.bool, device=gpu)
    inside[lo:hi] = True
    for new, old in ((flat.master, p0), (flat.shadow, s0)):
        assert torch.equal(_bits(new)[~inside], _bits(old)[~inside]), "written outside the range"
        changed = _bits(new) != _bits(old)
        assert not changed[pad].any()
        if new is flat.master:  # (an update below half a bf16 ulp leaves a shadow element as it was)
            assert changed[inside & ~pad].float().mean().item() > 0.99, "the range was not updated"
    assert torch.equal(flat.shadow[inside & ~pad], flat.master[inside & ~pad].to(torch.bfloat16))
    for new, old in ((flat.grad, g0), (m, m1), (v, v1)):
        assert torch.equal(_bits(new), _bits(old))
    # a range that cuts a chunk, a range outside the plan's, mismatched and misaligned buffers: errors, no launch
    snap = [t.clone() for t in (flat.master, flat.shadow, m, v, plan.partials_buf)]
    a = (HP["lr"], m, v, bc, HP["eps"], HP["weight_decay"])
    with pytest.raises(ValueError, match="cuts the chunk"):
        plan.apply(flat.offsets[6] + 8, hi, *a)
    half = LambPlan(flat, [(0, flat.offsets[5])])
    with pytest.raises(ValueError, match="cover"):
        half.apply(0, flat.total, *a)
    with pytest.raises(ValueError, match="numel"):
        plan.apply(lo, hi, HP["lr"], m[:-64], v, bc, HP["eps"], HP["weight_decay"])
    with pytest.raises(ValueError, match="numel"):
        plan.moments(0, m, v[:-64], bc, **MOM)
    lib = native.kernels()
    st = native.stream_handle()
    W, M, V, G, S = (t.data_ptr() for t in (flat.master, m, v, flat.grad, flat.shadow))
    T, N, PB, TR, BC = plan.table.data_ptr(), plan.n_chunks, plan.partials_buf.data_ptr(), plan.trust_dev.data_ptr(), \
        bc.data_ptr()
    gb = int(grad_dtype == torch.bfloat16)

    def moments(w=W, mm=M, vv=V, g=G, t=T, n=N, pb=PB, b=BC, clip=None):
        return lib.ddpx_lamb_moments(w, mm, vv, g, gb, t, n, None, pb, b, 0.9, 0.999, 1e-6, 0.01, 1.0, clip, st)

    def apply(w=W, mm=M, vv=V, s=S, t=T, n=N, tr=TR, lr=None, b=BC):
        return lib.ddpx_lamb_apply(w, mm, vv, s, t, n, tr, None, lr, 1e-2, b, 1e-6, 0.01, st)

    gmis = G + (4 if gb else 8)  # 8-B aligned passes for bf16 gradients, 16 B are required for fp32 ones
    for rc in (moments(w=W + 4), moments(mm=M + 8), moments(vv=V + 4), moments(g=gmis), moments(g=G + 2),
               moments(t=T + 8), moments(pb=PB + 2), moments(b=BC + 2), moments(clip=BC + 1), moments(w=None),
               moments(mm=None), moments(vv=None), moments(g=None), moments(t=None), moments(pb=None),
               moments(b=None),
               apply(w=W + 4), apply(mm=M + 8), apply(vv=V + 4), apply(s=S + 2), apply(s=S + 4), apply(t=T + 8),
               apply(tr=TR + 2), apply(lr=BC + 1), apply(b=BC + 2), apply(w=None), apply(mm=None), apply(vv=None),
               apply(t=None), apply(tr=None), apply(b=None)):
        assert rc != 0
    assert moments(n=0) == 0 and apply(n=0) == 0 and moments(n=-3) == 0 and apply(n=-3) == 0
    torch.cuda.synchronize()
    for new, old in zip((flat.master, flat.shadow, m, v, plan.partials_buf), snap):
        assert torch.equal(_bits(new), _bits(old))


# ----------------------------------------------------------------------------------------------- the optimizer
@pytest.mark.parametrize("max_norm", [None, 0.05], ids=["noclip", "clip"])
def test_captured_step_replays_equal_eager_steps(gpu, max_norm):
    """The training step captured as the trainer captures it (``capturable=True``): 3 replays of ONE captured step
    == the eager steps bit for bit in weights, both states, shadow, the trust table and the step counter; the table
    and the norm are recomputed on the device by every replay."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import LAMB
    from ddpx.runtime.graphs import try_capture
    from tests.test_gpu_lars import _torch_norm
    torch.manual_seed(5)
    a, b = MLP(hidden=256), MLP(hidden=256)
    b.load_state_dict(a.state_dict())
    for mdl in (a, b):
        ddpx.prepare_model(mdl, gpu)
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=max_norm)
    oa = LAMB(a.parameters(), capturable=True, **hp)
    ob = LAMB(b.parameters(), **hp)
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
            assert abs(nb[-1] - want) <= SUMSQ * want, (i, nb[-1], want)
    torch.cuda.synchronize()
    for x, y in zip(ta, tb[1:]):
        assert torch.equal(x, y)
    assert not torch.equal(ta[0], ta[1]) and not torch.equal(ta[1], ta[2])  # recomputed per replay
    fa, fb = oa.flat, ob.flat
    weights = [fa.index[id(p)] for p in a.parameters() if p.dim() > 1]
    assert all(ta[-1][j].item() != 1.0 for j in weights) and sum(t.item() == 1.0 for t in ta[-1]) == 3  # 3 biases
    assert na == nb[1:]
    assert oa.steps_taken() == 4 and ob.steps_taken() == 4 and torch.equal(oa.step_dev, ob.step_dev)
    assert torch.equal(fa.master, fb.master) and torch.equal(fa.shadow, fb.shadow)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    assert torch.equal(fa.shadow, fa.master.to(torch.bfloat16))
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


@pytest.mark.parametrize("variant,max_norm", [("overlap", None), ("overlap", 0.05), ("side", None), ("side", 0.05),
                                              ("zero1", None), ("zero1_comm", None)])
def test_replicated_ddp_with_bucket_overlap_is_bitwise_the_plain_step(gpu, pg, variant, max_norm):
    """World size 1, per-bucket optimizer overlap: the moments pass bucket by bucket, then the apply passes, on the
    compute stream (``overlap``) or the side stream (``side``); and ZeRO-1, whose one shard is the whole bucket, with
    the shard steps on the current stream (``zero1``) or the communicator stream (``zero1_comm``).  Buckets end at
    parameter boundaries and a parameter's chunks start at the parameter, so the chunk sums, hence all bits, are the
    single-process step's.  (Not so the clipped ZeRO-1 step: the SGD class's norm pass completes the global sum of
    squares in two roundings there, sharded buckets then replicated ones, so the clip factor may differ from the
    single-process one in its last bit; ``tests/test_gpu_lamb_multirank.py`` has that case.)"""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import LAMB
    from ddpx.parallel.comm import RcclComm
    from ddpx.parallel.ddp import DistributedDataParallel
    torch.manual_seed(0)
    a, b = MLP(hidden=512), MLP(hidden=512)
    b.load_state_dict(a.state_dict())
    ddpx.prepare_model(a, gpu)
    ddpx.prepare_model(b, gpu)
    comm = RcclComm(gpu)
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=max_norm)
    oa = LAMB(a.parameters(), **hp)
    shard = variant.startswith("zero1")
    da = DistributedDataParallel(a, comm=comm, bucket_cap_mb=1.0, first_bucket_mb=0.25, reduce_single=True,
                                 overlap_optimizer=True, shard_optimizer=shard,
                                 side_stream_optimizer=variant == "side", comm_side_optimizer=variant == "zero1_comm")
    assert len(da.bucket_ranges) >= 2 and da.sharded == shard
    assert (da.optimizer_stream() is not None) == (variant == "zero1_comm")
    da.attach_optimizer(oa)
    ob = LAMB(b.parameters(), **hp)
    x = torch.rand(256, 3072, device=gpu).to(torch.bfloat16)
    t = torch.randint(0, 10, (256,), device=gpu)
    for _ in range(3):
        for net, opt in ((da, oa), (b, ob)):
            opt.zero_grad()
            loss, _ = net.forward_loss(x, t)
            loss.backward()
            opt.step()
    torch.cuda.synchronize()
    assert len(oa._lamb_plan.ranges) >= len(da.bucket_ranges)  # the per-bucket / per-shard path ran
    assert len(ob._lamb_plan.ranges) == 1
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    fa, fb = oa.flat, ob.flat
    for p, q in zip(a.parameters(), b.parameters()):
        i, j = fa.index[id(p)], fb.index[id(q)]
        assert oa.trust_ratio_dev[i] == ob.trust_ratio_dev[j]
        assert (oa.trust_ratio_dev[i].item() == 1.0) == (p.dim() <= 1)
        assert torch.equal(oa.exp_avg[fa.slice(i)], ob.exp_avg[fb.slice(j)])
        assert torch.equal(oa.exp_avg_sq[fa.slice(i)], ob.exp_avg_sq[fb.slice(j)])
    assert oa.steps_taken() == 3 and ob.steps_taken() == 3
    da.close()
    comm.close()


def _fill_but(flat, seed, skip=None, scale=0.5):
    """``_fill`` that leaves out parameter ``skip``: nobody produces a gradient for it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat.grad.fill_(float("nan"))
    out = []
    for i, p in enumerate(flat.params):
        gi = (torch.randn(p.shape, generator=g) * scale).to(flat.device)
        if i == skip:
            out.append(None)
            continue
        p.main_grad.copy_(gi)
        flat.grad_done(p)
        out.append(p.main_grad.detach().clone())
    return out


@GD
def test_a_parameter_without_gradient_is_left_alone(gpu, grad_dtype):
    """Parameter X gets no gradient in step 2 of 3: it keeps w, m and v bit for bit in that step and its ratio reads 1.
    Without clipping no other parameter's update depends on X, so all the others equal, bit for bit, a run in which
    X does get its gradient; and everything stays within the bounds of the fp64 loop that skips X."""
    import warnings
    from ddpx.optim import LAMB
    from ddpx.runtime.flat_params import FlatParams
    X = 7  # (128, 256): two chunks

    def make():
        torch.manual_seed(21)
        mdl = _Odd(_shapes()).to(gpu)
        return mdl, FlatParams(mdl, grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)

    (ma, fa), (mb, fb) = make(), make()
    oa, ob = LAMB(ma.parameters(), **HP), LAMB(mb.parameters(), **HP)
    params = list(fa.params)
    ref = LambFp64(params, **HP)
    for step in range(3):
        skip = X if step == 1 else None
        before = [t[fa.slice(X)].clone() for t in (fa.master, oa.exp_avg, oa.exp_avg_sq, fa.shadow)]
        grads = _fill_but(fa, 60 + step, skip)
        _fill_but(fb, 60 + step, None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "parameters without gradient this step"
            oa.step()
        ob.step()
        oa.zero_grad()
        ob.zero_grad()
        ref.step(grads)
        if skip is not None:
            after = [t[fa.slice(X)] for t in (fa.master, oa.exp_avg, oa.exp_avg_sq, fa.shadow)]
            for x, y in zip(before, after):
                assert torch.equal(_bits(x), _bits(y))
            assert oa.trust_ratio_dev[X].item() == 1.0 and ob.trust_ratio_dev[X].item() != 1.0
        if step <= 1:
            for i in range(len(params)):
                if i == X and step == 1:
                    continue
                sl = fa.slice(i)
                assert oa.trust_ratio_dev[i] == ob.trust_ratio_dev[i]
                for x, y in ((fa.master, fb.master), (oa.exp_avg, ob.exp_avg), (oa.exp_avg_sq, ob.exp_avg_sq)):
                    assert torch.equal(x[sl], y[sl]), (step, i)
    for i in range(len(params)):  # the last step too, for everybody but X (whose history differs)
        if i != X:
            assert torch.equal(fa.master[fa.slice(i)], fb.master[fb.slice(i)])
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(params):
        sl = fa.slice(i)
        worst = [max(a, b) for a, b in zip(worst, ref.check(i, p, oa.exp_avg[sl], oa.exp_avg_sq[sl], "skipped"))]
    print(f"3 steps, one skipped {grad_dtype}: achieved fraction of the bound: param {worst[0]:.3f} "
          f"exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")
    assert oa.steps_taken() == 3


def _twin_lamb_step(params, ms, vs, hp, t):
    """The reference LAMB in plain fp32 torch ops, parameter by parameter."""
    b1, b2 = hp["betas"]
    bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    with torch.no_grad():
        for p, m, v in zip(params, ms, vs):
            g = p.grad
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (m / bc1) / (v.sqrt() / bc2s + hp["eps"]) + hp["weight_decay"] * p
            wn, un = p.norm(), u.norm()
            tr = 1.0
            if p.dim() > 1 and wn > 0 and un > 0:
                tr = wn / un
            p.sub_(hp["lr"] * tr * u)


def test_whole_model_tracks_a_torch_fp32_twin(gpu):
    """``--model mlp --hidden 256 --batch_size 128 --dtype bf16 --optimizer lamb`` built as the training scripts
    build it, 6 steps on one batch against a torch fp32 twin that runs the reference LAMB from the same init, within
    the tolerance ``smoke()`` uses for its SGD twin (3 % + 0.02 on every loss)."""
    from ddpx.models import MLP
    from ddpx.optim import LAMB
    from ddpx.train.app import build_model_and_optimizer, build_parser
    torch.manual_seed(0)
    args = build_parser("t").parse_args(["1", "1", "--model", "mlp", "--hidden", "256", "--batch_size", "128",
                                         "--dtype", "bf16", "--kernels", "native", "--optimizer", "lamb"])
    model, opt = build_model_and_optimizer(args, gpu)
    assert type(opt) is LAMB and model.use_native and opt.flat.fused_opt is None and not opt.fused_active()
    twin = MLP(hidden=256, layers=3)
    twin.load_state_dict(model.state_dict())
    twin = twin.to(gpu)
    twin.use_native = False
    twin.compute_dtype = torch.float32
    g = opt.param_groups[0]
    hp = {k: g[k] for k in ("lr", "betas", "eps", "weight_decay")}
    assert hp == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    tparams = list(twin.parameters())
    ms, vs = [torch.zeros_like(p) for p in tparams], [torch.zeros_like(p) for p in tparams]
    w0 = [p.detach().clone() for p in model.parameters()]
    x = torch.rand(128, 3072, device=gpu).to(torch.bfloat16)
    y = torch.randint(0, 10, (128,), device=gpu)
    losses, ref = [], []
    for step in range(6):
        opt.zero_grad()
        loss, _ = model.forward_loss(x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        for p in tparams:
            p.grad = None
        tl = torch.nn.functional.cross_entropy(twin(x.float()), y)
        tl.backward()
        _twin_lamb_step(tparams, ms, vs, hp, step + 1)
        ref.append(float(tl.item()))
    print("lamb losses", losses, "torch fp32 twin", ref)
    assert all(math.isfinite(v) for v in losses), losses
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 0.03 * abs(b) + 0.02, (losses, ref)
    f = opt.flat
    for p, p0 in zip(model.parameters(), w0):
        assert not torch.equal(p.detach(), p0)
        assert (opt.trust_ratio_dev[f.index[id(p)]].item() == 1.0) == (p.dim() <= 1)
    assert opt.flat.fused_opt is None and opt.steps_taken() == 6


def test_full_checkpoint_round_trip(gpu, tmp_path):
    """3 steps, save, continue in a fresh model + optimizer loaded from the file: the next 2 steps are bitwise the
    uninterrupted run's (weights, both states, shadow, trust table); foreign files are refused both ways."""
    from ddpx.optim import LAMB, LARS, SGD, AdamW
    from ddpx.runtime.flat_params import FlatParams
    from ddpx.train.checkpoint import load_full_checkpoint, save_full_checkpoint
    path = str(tmp_path / "full.pt")

    def make(seed):
        torch.manual_seed(seed)
        m = _Odd(_shapes()).to(gpu)
        return m, FlatParams(m, shadow_dtype=torch.bfloat16)

    m, flat = make(13)
    opt = LAMB(m.parameters(), max_grad_norm=5.0, **HP)
    for step in range(5):
        if step == 3:
            save_full_checkpoint(path, m, opt, None, epoch=0)
        opt.zero_grad()
        _fill(flat, 40 + step)
        opt.step()
    m2, flat2 = make(99)  # another init: everything must come from the file
    opt2 = LAMB(m2.parameters(), lr=0.5, betas=(0.5, 0.5), weight_decay=0.5, eps=1.0, exclude_1d=False,
                max_grad_norm=5.0)
    assert load_full_checkpoint(path, m2, opt2, None, map_location=gpu) == 1
    assert opt2.steps_taken() == 3 and opt2.param_groups[0]["exclude_1d"] is True
    assert opt2.param_groups[0]["betas"] == HP["betas"] and opt2.param_groups[0]["eps"] == HP["eps"]
    for step in (3, 4):
        opt2.zero_grad()
        _fill(flat2, 40 + step)
        opt2.step()
    for i in range(len(flat.params)):
        sl = flat.slice(i)
        for a, b in ((flat.master, flat2.master), (flat.shadow, flat2.shadow), (opt.exp_avg, opt2.exp_avg),
                     (opt.exp_avg_sq, opt2.exp_avg_sq)):
            assert torch.equal(a[sl], b[sl]), i
    assert torch.equal(opt.trust_ratio_dev, opt2.trust_ratio_dev) and (opt.trust_ratio_dev != 1).sum() >= 4
    assert torch.equal(opt.grad_norm_dev, opt2.grad_norm_dev) and torch.equal(opt.step_dev, opt2.step_dev)
    # the other optimizers' files are refused, and they refuse this one
    others = {"sgd": lambda ps: SGD(ps, lr=0.1, momentum=0.9), "adamw": lambda ps: AdamW(ps),
              "lars": lambda ps: LARS(ps, lr=0.1)}
    for name, mk in others.items():
        m3, f3 = make(1)
        o3 = mk(m3.parameters())
        with pytest.raises(ValueError, match="another optimizer"):
            load_full_checkpoint(path, m3, o3, None, map_location=gpu)
        _fill(f3, 7)
        o3.step()
        theirs = str(tmp_path / f"{name}.pt")
        save_full_checkpoint(theirs, m3, o3, None, epoch=0)
        m4, _ = make(2)
        with pytest.raises(ValueError, match="another optimizer"):
            load_full_checkpoint(theirs, m4, LAMB(m4.parameters(), **HP), None, map_location=gpu)
