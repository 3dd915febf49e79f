"""Parameter groups on the GPU: the entry points with the hyper table (``ddpx_sgd_flat_chunks``,
``ddpx_adamw_flat_hyper``, ``ddpx_lars_trust``, ``ddpx_lamb_moments`` / ``ddpx_lamb_apply``) against the scalar kernels
they extend, and the four optimizers with two groups.

The kernel-level oracles are exact.  A table whose rows are all ``{1, wd}`` must give the scalar entry point's bits;
a non-uniform table must give, parameter by parameter, the bits of the scalar kernel launched on that parameter's
slice alone with ``weight_decay = wd_i`` and ``lr_host = fp32(lr_0) * fp32(lr_mul_i)``, one fp32 product formed on
the host as the kernel forms it on the device.  All on ONE synthetic store: ``[3, 32771]`` (three full 32768-element
chunks and a 9-element last chunk with ``len % 4 == 1``), ``[7]``, ``[1]``, ``[130, 257]``, ``[64]``, fp32 and bf16
gradients, NaN in every padding element.

LARS and LAMB with per-parameter ``wd`` and ``adapt`` run 3 steps against the fp64 loops of ``tests/_groups_ref.py``
(the bounds of ``tests/_lars_ref.py`` / ``tests/_lamb_ref.py``, k = 1) and against the CPU path of the same optimizer
(k = 2), which must lie within the sum of the two bounds.  Where ``lr_mul != 1`` the kernels spend ONE more rounding
than the files count, the product ``lr * lr_mul`` (``k_lr = 1``); the multiplier itself is an input, as lr is.
"""
import copy

import pytest
import torch

from tests._groups_ref import LambGroupsFp64, LarsGroupsFp64
from tests._lars_ref import TINY, U, f32

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32771), (7,), (1,), (130, 257), (64,)]
WD = [5e-4, 0.0, 0.0, 1e-3, 0.0]      # per parameter
MUL = [1.0, 0.1, 0.1, 1.0, 0.25]      # per parameter (rounded to fp32 below)
GD = pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
BETAS, EPS = (0.9, 0.999), 1e-8


class _Odd(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s) * 0.1) for s in shapes])


def _hyper(flat, mul, wd):
    from ddpx.optim.flat import Hyper
    mul = [f32(x) for x in mul]
    table = torch.tensor(list(zip(mul, wd)), dtype=torch.float32).reshape(-1, 2).to(flat.device)
    return Hyper([0] * len(mul), mul, [float(w) for w in wd], False, table)


def _store(gpu, grad_dtype, seed=0):
    """The synthetic store with random gradients and states and NaN in every padding element; returns
    ``(flat, pad, states)`` with states = {momentum, exp_avg, exp_avg_sq} (store-sized)."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    flat = FlatParams(_Odd(SHAPES).to(gpu), grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)
    pad = torch.ones(flat.total, dtype=torch.bool, device=gpu)
    for o, n in zip(flat.offsets, flat.numels):
        pad[o:o + n] = False
    assert pad.any() and sorted(flat.numels) == sorted(a * b for a, b in ((*s, 1)[:2] for s in SHAPES))
    st = {"momentum": torch.randn(flat.total, device=gpu) * 0.05, "exp_avg": torch.randn(flat.total, device=gpu) * 0.01,
          "exp_avg_sq": (torch.randn(flat.total, device=gpu) * 0.01).square()}
    nan = float("nan")
    for t in (flat.master, flat.shadow, *st.values()):
        t[pad] = nan
    g = torch.Generator(device="cpu").manual_seed(seed + 100)
    flat.grad.fill_(nan)
    for p in flat.params:
        p.main_grad.copy_((torch.randn(p.shape, generator=g) * 0.5).to(gpu))
        flat.grad_done(p)
    return flat, pad, st


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bc(gpu, t=3):
    from ddpx.ops.elementwise import adamw_advance_
    counter = torch.full((1,), t - 1, dtype=torch.int32, device=gpu)
    bc = torch.zeros(2, device=gpu)
    adamw_advance_(counter, bc, *BETAS)
    return bc


def _scalar_by_slice(kind, flat, p0, s0, st0, bc, lrs, wds, clip, nesterov=False):
    """The scalar kernel (``ddpx_sgd_flat`` / ``ddpx_adamw_flat``) launched on every parameter's slice alone;
    returns clones of master, shadow and the states after it.  ``lrs[i]``: a float or a 0-d device tensor."""
    from ddpx.ops.elementwise import adamw_flat_, sgd_flat_
    p, s = p0.clone(), s0.clone()
    st = {k: v.clone() for k, v in st0.items()}
    for i in range(len(flat.params)):
        sl = flat.slice(i)
        if kind == "sgd":
            sgd_flat_(p[sl], st["momentum"][sl], flat.grad[sl], s[sl], lrs[i], 0.9, wds[i], nesterov=nesterov, clip=clip)
        else:
            adamw_flat_(p[sl], st["exp_avg"][sl], st["exp_avg_sq"][sl], flat.grad[sl], s[sl], lrs[i], bc, None, *BETAS,
                        EPS, wds[i], clip=clip)
    return p, s, st


def _table_driven(kind, plan, hyper, st, bc, lr, clip, start=None, end=None, nesterov=False):
    flat = plan.flat
    start, end = (0 if start is None else start), (flat.total if end is None else end)
    if kind == "sgd":
        plan.sgd_update(start, end, hyper, lr, 0.9, nesterov=nesterov, clip=clip, momentum_buf=st["momentum"])
    else:
        plan.adamw_update(start, end, hyper, lr, st["exp_avg"], st["exp_avg_sq"], bc, *BETAS, EPS, clip=clip)


def _assert_equal_everywhere(flat, pad, st, want, what):
    p, s, wst = want
    for name, got, ref in (("master", flat.master, p), ("shadow", flat.shadow, s),
                           *((k, st[k], wst[k]) for k in st)):
        assert torch.equal(_bits(got)[~pad], _bits(ref)[~pad]), (what, name)
        assert torch.isnan(got[pad].float()).all(), (what, name, "a padding element was written")
    assert torch.equal(flat.shadow[~pad], flat.master[~pad].to(torch.bfloat16)), what


@GD
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_uniform_table_gives_the_scalar_kernels_bits(gpu, grad_dtype, kind):
    from ddpx.ops.lars import PidChunkPlan
    flat, pad, st = _store(gpu, grad_dtype, seed=1)
    p0, s0, st0 = flat.master.clone(), flat.shadow.clone(), {k: v.clone() for k, v in st.items()}
    plan, bc = PidChunkPlan(flat), _bc(gpu)
    assert plan.n_chunks == 4 + 1 + 1 + 2 + 1 and sorted(c[1] for c in plan.chunks)[:4] == [1, 7, 9, 64]
    n = len(SHAPES)
    for nesterov in ((False, True) if kind == "sgd" else (False,)):
        for clip in (None, torch.tensor(0.37, device=gpu)):
            flat.master.copy_(p0)
            flat.shadow.copy_(s0)
            for k in st:
                st[k].copy_(st0[k])
            _table_driven(kind, plan, _hyper(flat, [1.0] * n, [5e-4] * n), st, bc, 0.4, clip, nesterov=nesterov)
            want = _scalar_by_slice(kind, flat, p0, s0, st0, bc, [0.4] * n, [5e-4] * n, clip, nesterov)
            _assert_equal_everywhere(flat, pad, st, want, (kind, nesterov, clip is not None))
            assert not torch.equal(flat.master[~pad], p0[~pad])


@GD
@pytest.mark.parametrize("dev_lr", [False, True], ids=["host_lr", "device_lr"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_non_uniform_table_is_the_scalar_kernel_slice_by_slice(gpu, grad_dtype, kind, dev_lr):
    from ddpx.ops.lars import PidChunkPlan
    flat, pad, st = _store(gpu, grad_dtype, seed=2)
    p0, s0, st0 = flat.master.clone(), flat.shadow.clone(), {k: v.clone() for k, v in st.items()}
    plan, bc = PidChunkPlan(flat), _bc(gpu)
    hyper = _hyper(flat, MUL, WD)
    lr0 = torch.tensor(0.4, dtype=torch.float32)
    lrs = [float(lr0 * torch.tensor(m, dtype=torch.float32)) for m in hyper.lr_mul]  # ONE fp32 product each
    clip = torch.tensor(0.61, device=gpu)
    _table_driven(kind, plan, hyper, st, bc, lr0.to(gpu) if dev_lr else 0.4, clip)
    want = _scalar_by_slice(kind, flat, p0, s0, st0, bc, lrs, WD, clip)
    _assert_equal_everywhere(flat, pad, st, want, (kind, dev_lr))
    # (the rows matter: the scalar kernel with group 0's values everywhere gives other bits)
    other = _scalar_by_slice(kind, flat, p0, s0, st0, bc, [0.4] * 5, [5e-4] * 5, clip)
    assert not torch.equal(other[0][flat.slice(1)], flat.master[flat.slice(1)])


@GD
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_sub_range_launch_leaves_everything_else_alone(gpu, grad_dtype, kind):
    """Parameters 1 .. 3 only, every buffer outside them filled with a sentinel pattern's bits before."""
    from ddpx.ops.lars import PidChunkPlan
    flat, pad, st = _store(gpu, grad_dtype, seed=3)
    inside = torch.zeros(flat.total, dtype=torch.bool, device=gpu)
    lo, hi = flat.offsets[1], flat.offsets[4]
    inside[lo:hi] = True
    for t in (flat.master, flat.shadow, *st.values()):
        t[~inside] = 3.0  # the sentinel; the padding inside the range keeps its NaN
    g0 = flat.grad.clone()
    p0, s0, st0 = flat.master.clone(), flat.shadow.clone(), {k: v.clone() for k, v in st.items()}
    _table_driven(kind, PidChunkPlan(flat), _hyper(flat, MUL, WD), st, _bc(gpu), 0.4, None, lo, hi)
    used = ("momentum",) if kind == "sgd" else ("exp_avg", "exp_avg_sq")
    for new, old, written in ((flat.master, p0, True), (flat.shadow, s0, True),
                              *((st[k], st0[k], k in used) for k in st)):
        assert torch.equal(_bits(new)[~inside], _bits(old)[~inside]), "written outside the range"
        changed = _bits(new) != _bits(old)
        assert not changed[pad].any(), "a padding element was written"
        if written and new is not flat.shadow:
            assert changed[inside & ~pad].float().mean().item() > 0.99, "the range was not updated"
        if not written:
            assert not changed.any()
    assert torch.equal(_bits(flat.grad), _bits(g0))


def test_refused_pointers_and_empty_tables(gpu):
    from ddpx.ops.lars import LarsPlan
    from ddpx.runtime import native
    flat, pad, st = _store(gpu, torch.float32, seed=4)
    plan = LarsPlan(flat)
    hyper = _hyper(flat, MUL, WD).table
    snap = [t.clone() for t in (flat.master, flat.shadow, *st.values(), plan.trust_dev)]
    lib, s = native.kernels(), native.stream_handle()
    P, M, V, G, SH = (flat.master.data_ptr(), st["momentum"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                      flat.grad.data_ptr(), flat.shadow.data_ptr())
    T, N, H, TR, BC = plan.table.data_ptr(), plan.n_chunks, hyper.data_ptr(), plan.trust_dev.data_ptr(), _bc(gpu)
    A = st["exp_avg"].data_ptr()

    def sgd(p=P, b=M, g=G, t=T, n=N, tr=TR, h=H):
        return lib.ddpx_sgd_flat_chunks(p, b, g, 0, SH, t, n, tr, h, None, 0.4, 0.9, 0.0, 1.0, None, 0, 0, s)

    def adamw(p=P, t=T, n=N, h=H, bc=BC.data_ptr()):
        return lib.ddpx_adamw_flat_hyper(p, A, V, G, 0, SH, t, n, h, None, 1e-3, bc, 0.9, 0.999, 1e-8, 1.0, None, s)

    def trust(h=H, n=plan.P):
        return lib.ddpx_lars_trust(plan.sq.data_ptr(), plan.plain.data_ptr(), h, n, 1e-3, 0.0, 1e-8, 0.0, None, TR, s)

    def moments(t=T, n=N, h=H):
        return lib.ddpx_lamb_moments(P, A, V, G, 0, t, n, h, plan.partials_buf.data_ptr(), BC.data_ptr(), 0.9,
                                     0.999, 1e-6, 0.0, 1.0, None, s)

    def apply(t=T, n=N, h=H, tr=TR):
        return lib.ddpx_lamb_apply(P, A, V, SH, t, n, tr, h, None, 1e-3, BC.data_ptr(), 1e-6, 0.0, s)

    for fn in (sgd, adamw, moments, apply):
        assert fn(h=H + 4) == -1 and fn(t=None) == -1 and fn(t=T + 8) == -1, fn.__name__
        assert fn(n=0) == 0, fn.__name__
    # a null table: refused where the pass has no scalar form behind the same entry point (the others then run
    # that form, which test_lars_and_lamb_tables_with_one_wd_give_the_scalar_entry_points_bits compares)
    assert adamw(h=None) == -1 and sgd(h=None, tr=None) == -1
    assert trust(h=H + 4) == -1 and trust(n=0) == 0
    assert sgd(p=P + 4) == -1 and sgd(b=None) == -1 and sgd(g=G + 4) == -1 and sgd(tr=TR + 2) == -1
    assert adamw(p=P + 4) == -1 and adamw(bc=None) == -1 and apply(tr=None) == -1
    torch.cuda.synchronize()
    for new, old in zip((flat.master, flat.shadow, *st.values(), plan.trust_dev), snap):
        assert torch.equal(_bits(new), _bits(old)), "a refused or empty launch wrote something"


@GD
def test_lars_and_lamb_tables_with_one_wd_give_the_scalar_entry_points_bits(gpu, grad_dtype):
    from ddpx.ops.lamb import LambPlan
    from ddpx.ops.lars import LarsPlan
    flat, pad, st = _store(gpu, grad_dtype, seed=5)
    n = len(SHAPES)
    hyper = _hyper(flat, [1.0] * n, [5e-4] * n)
    p0, s0, st0 = flat.master.clone(), flat.shadow.clone(), {k: v.clone() for k, v in st.items()}

    def reset():
        flat.master.copy_(p0)
        flat.shadow.copy_(s0)
        for k in st:
            st[k].copy_(st0[k])
    # LARS: the trust table, then the update
    res = torch.zeros(3, device=gpu)
    plan = LarsPlan(flat, result=res)
    out = []
    for h in (None, hyper):
        reset()
        for k in range(len(plan.ranges)):
            plan.partials(k)
        plan.reduce()
        plan.trust(1e-3, 5e-4, 1e-8, 5.0, hyper=h)
        plan.update(0, flat.total, 0.4, 0.9, 5e-4, clip=plan.coef_dev, momentum_buf=st["momentum"], hyper=h)
        out.append([t.clone() for t in (plan.trust_dev, res, flat.master, flat.shadow, st["momentum"])])
    assert sum(t != 1.0 for t in out[0][0].tolist()) == 2
    for a, b in zip(*out):
        assert torch.equal(_bits(a), _bits(b))
    # LAMB: the moments pass with its per-chunk partials, then the apply pass
    lplan, bc = LambPlan(flat), _bc(gpu)
    out = []
    for h in (None, hyper):
        reset()
        lplan.compute(st["exp_avg"], st["exp_avg_sq"], bc, BETAS, 1e-6, 5e-4, clip=res[2], hyper=h)
        parts = lplan.partials_buf.clone()
        lplan.apply(0, flat.total, 1e-2, st["exp_avg"], st["exp_avg_sq"], bc, 1e-6, 5e-4, hyper=h)
        out.append([parts, lplan.trust_dev.clone(), flat.master.clone(), flat.shadow.clone(), st["exp_avg"].clone(),
                    st["exp_avg_sq"].clone()])
    for a, b in zip(*out):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(out[0][2][~pad], p0[~pad]) and torch.isnan(flat.master[pad]).all()


def _two_stores(gpu, grad_dtype, seed):
    """The same parameters in a GPU store and a CPU store (fp32 or bf16 gradient buffers)."""
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    cm = _Odd(SHAPES)
    gm = copy.deepcopy(cm).to(gpu)
    return (gm, FlatParams(gm, grad_dtype=grad_dtype, shadow_dtype=torch.bfloat16)), (cm, FlatParams(cm, grad_dtype=grad_dtype))


def _fill_both(stores, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _, flat in stores:
        flat.grad.fill_(float("nan"))
    grads = []
    for ps in zip(*(m.parameters() for m, _ in stores)):
        x = torch.randn(ps[0].shape, generator=g) * 0.5
        for p, (_, flat) in zip(ps, stores):
            p.main_grad.copy_(x.to(flat.device))
            flat.grad_done(p)
        grads.append(ps[1].main_grad.detach().float().clone())  # (as the buffer holds it: bf16-rounded with g16)
    return grads


def _split(model, lrs, wds, **second):
    ps = list(model.parameters())  # group 1: the [7], the [130, 257] and the [64]
    return [{"params": [ps[0], ps[2]], "lr": lrs[0], "weight_decay": wds[0]},
            {"params": [ps[1], ps[3], ps[4]], "lr": lrs[1], "weight_decay": wds[1], **second}]


@GD
@pytest.mark.parametrize("second", [dict(), dict(adapt=False)], ids=["adapt", "adapt_off"])
@pytest.mark.parametrize("name", ["LARS", "LAMB"])
def test_lars_and_lamb_groups_match_fp64_and_the_cpu_path(gpu, grad_dtype, name, second):
    import ddpx.optim
    cls = getattr(ddpx.optim, name)
    stores = _two_stores(gpu, grad_dtype, seed=6)
    lars = name == "LARS"
    lrs, wds = ((0.4, 0.04), (5e-4, 0.0)) if lars else ((1e-2, 1e-3), (0.01, 0.0))
    hp = dict(momentum=0.9, trust_coef=1e-3, eps=1e-8) if lars else dict(betas=BETAS, eps=1e-6)
    opts = [cls(_split(m, lrs, wds, **second), lr=9.0, max_grad_norm=5.0, allow_groups=True, **hp) for m, _ in stores]
    params = list(stores[1][0].parameters())
    grp = [0, 1, 0, 1, 1]
    adapt = [p.dim() > 1 and (g == 0 or second.get("adapt", True)) for p, g in zip(params, grp)]
    mk = LarsGroupsFp64 if lars else LambGroupsFp64
    # the kernels: k = 1, and one more rounding (lr_0 * lr_mul) where the multiplier is not 1; the CPU path: k = 2
    # and the group's own rate.  The reference of the kernels takes the exact product of the two fp32 factors.
    lr_gpu = [f32(lrs[0]) * (1.0 if g == 0 else f32(lrs[1] / lrs[0])) for g in grp]
    refs = [mk(params, lr_gpu, [wds[g] for g in grp], adapt, exclude_1d=False, max_grad_norm=5.0, k=1,
               k_lr=[int(g != 0) for g in grp], **hp),
            mk(params, [f32(lrs[g]) for g in grp], [wds[g] for g in grp], adapt, exclude_1d=False, max_grad_norm=5.0,
               k=2, **hp)]
    for step in range(3):
        grads = _fill_both(stores, 40 + step)
        for o, r in zip(opts, refs):
            o.step()
            o.zero_grad()
            r.step(grads)
    assert refs[0].coef < 1.0, "the clip must be active"
    assert not opts[0]._hyper().uniform and opts[0]._hyper().table is not None
    worst = 0.0
    for o, r, (m, flat) in zip(opts, refs, stores):
        for i, p in enumerate(m.parameters()):
            sl = flat.slice(flat.index[id(p)])
            t = o.trust_ratio_dev[flat.index[id(p)]].item()
            assert (t != 1.0) == adapt[i], (name, i, t)
            if lars:
                worst = max(worst, *r.check(i, p, o.momentum_buffer[sl], flat.device.type))
            else:
                worst = max(worst, *r.check(i, p, o.exp_avg[sl], o.exp_avg_sq[sl], flat.device.type))
    # GPU against the CPU path: within the sum of the two bounds (+ the two references' own distance: their rates
    # differ by the rounding the k_lr term counts)
    for i, (p, q) in enumerate(zip(stores[0][0].parameters(), params)):
        d = (p.detach().double().cpu() - q.detach().double()).abs()
        bound = refs[0].Ep[i] + refs[1].Ep[i] + (refs[0].P[i] - refs[1].P[i]).abs() + TINY
        assert (d <= bound).all(), (name, i, (d / bound).max().item())
    f = stores[0][1]
    for i in range(len(f.params)):
        assert torch.equal(f.shadow[f.slice(i)], f.master[f.slice(i)].to(torch.bfloat16))
    print(f"{name} groups {second} {grad_dtype}: worst achieved fraction of the fp64 bounds {worst:.3f}")


# ------------------------------------------------------------------ the optimizers on the toy MLP
def _mlp_pair(gpu, seed):
    import ddpx
    from ddpx.models import MLP
    torch.manual_seed(seed)
    model = MLP(hidden=512)
    twin = [torch.nn.Parameter(p.detach().clone().to(gpu)) for p in model.parameters()]
    ddpx.prepare_model(model, gpu)
    return model, twin


def _mlp_groups(params, wd, lr):
    from ddpx.optim import decay_groups
    g = decay_groups(params, wd)
    g[1]["lr"] = lr / 10
    return g


def _mlp_steps(gpu, model, opt, twin, topt, steps, on_step):
    for s in range(steps):
        gen = torch.Generator(device="cpu").manual_seed(900 + s)
        x = torch.rand(128, 3072, generator=gen).to(gpu).to(torch.bfloat16)
        y = torch.randint(0, 10, (128,), generator=gen).to(gpu)
        opt.zero_grad()
        loss, _ = model.forward_loss(x, y)
        loss.backward()
        grads = [p.main_grad.detach().float().clone() for p in model.parameters()]
        for q, g in zip(twin, grads):
            q.grad = g.view_as(q).clone()
        opt.step()
        topt.step()
        on_step(grads)


def test_five_eager_steps_of_two_group_adamw_match_torch(gpu):
    """``test_five_eager_steps_match_torch_adamw``'s bound (``tests/test_gpu_adamw.py``'s ``_Fp64Run`` with k = the
    kernel's counts + torch's), parameter by parameter with its group's lr and wd.  Group 1's rate reaches the kernel
    as fp32(lr_0) * fp32(0.1): the two inputs' roundings, the product's and the reference's own fp32(lr_1) are at
    most 4 u apart, which moves decay and step size like 4 more roundings of p: k_p + 4 there."""
    from ddpx.optim import AdamW
    from tests.test_gpu_adamw import K_M, K_P, K_V, T_M, T_P, T_V, _Fp64Run
    model, twin = _mlp_pair(gpu, seed=21)
    lr, wd = 1e-3, 0.01
    opt = AdamW(_mlp_groups(model, wd, lr), lr=lr, betas=BETAS, eps=EPS, allow_groups=True)
    topt = torch.optim.AdamW(_mlp_groups(twin, wd, lr), lr=lr, betas=BETAS, eps=EPS)
    assert not opt._hyper().uniform
    runs = []
    for p in model.parameters():
        one_d = p.dim() <= 1
        hp = dict(lr=lr / 10 if one_d else lr, betas=BETAS, eps=EPS, weight_decay=0.0 if one_d else wd)
        runs.append(_Fp64Run([p], hp, (K_M + T_M, K_V + T_V, K_P + T_P + (4 if one_d else 0))))

    def on_step(grads):
        bc = opt._bc_dev.double().tolist()
        for r, g in zip(runs, grads):
            r.step([g.view_as(r.P[0])], r.hp["lr"], bc)
    _mlp_steps(gpu, model, opt, twin, topt, 5, on_step)
    assert opt.steps_taken() == 5 and not opt.fused_active()
    sd = opt.state_dict()["state"]
    order = [p for g in opt.param_groups for p in g["params"]]
    torder = [q for g in topt.param_groups for q in g["params"]]
    by_param = {id(p): (sd[i], topt.state[q], q) for i, (p, q) in enumerate(zip(order, torder))}
    worst = [0.0] * 3
    for p, r in zip(model.parameters(), runs):
        mine, theirs, q = by_param[id(p)]
        trip_o = (mine["exp_avg"], mine["exp_avg_sq"], p.detach())
        trip_t = (theirs["exp_avg"], theirs["exp_avg_sq"], q.detach())
        for j, (a, b, bound) in enumerate(zip(trip_o, trip_t, r.bounds(0))):
            d = (a.double() - b.double()).abs().view_as(bound)
            assert torch.isfinite(a).all() and (d <= bound).all(), ("mvp"[j], tuple(p.shape), (d / bound).max().item())
            worst[j] = max(worst[j], (d / bound).max().item())
    print(f"two-group AdamW, 5 eager steps: |ours - torch| / bound (m, v, p) = {[round(x, 3) for x in worst]}")


def test_five_eager_steps_of_two_group_sgd_match_torch(gpu):
    """SGD has no ``_Fp64Run``; the same construction with ``tests/_lars_ref.py``'s bounds (no parameter adapts: plain
    SGD): ours within the fp64 loop's k = 1 bound (+ 1 rounding of the rate in group 1, ``k_lr``), torch's fp32 GPU
    SGD within its k = 2 bound (mul + add per fma), so the two are within the sum."""
    from ddpx.optim import SGD
    model, twin = _mlp_pair(gpu, seed=22)
    lr, wd = 0.1, 5e-4
    opt = SGD(_mlp_groups(model, wd, lr), lr=lr, momentum=0.9, allow_groups=True)
    topt = torch.optim.SGD(_mlp_groups(twin, wd, lr), lr=lr, momentum=0.9)
    assert not opt.fused_active() and opt.flat.fused_opt is None
    params = list(model.parameters())
    one_d = [p.dim() <= 1 for p in params]
    wds = [0.0 if o else wd for o in one_d]
    none = [False] * len(params)
    cpu = [p.detach().cpu() for p in params]
    ours = LarsGroupsFp64(cpu, [f32(lr) * f32(0.1) if o else f32(lr) for o in one_d], wds, none, k=1,
                          k_lr=[int(o) for o in one_d])
    theirs = LarsGroupsFp64(cpu, [f32(lr / 10) if o else f32(lr) for o in one_d], wds, none, k=2)

    def on_step(grads):
        shaped = [g.view_as(p).cpu() for g, p in zip(grads, params)]
        ours.step(shaped)
        theirs.step(shaped)
    _mlp_steps(gpu, model, opt, twin, topt, 5, on_step)
    f = opt.flat
    for i, (p, q) in enumerate(zip(params, twin)):
        ours.check(i, p, opt.momentum_buffer[f.slice(f.index[id(p)])], "ours")
        theirs.check(i, q, topt.state[q]["momentum_buffer"], "torch")
        d = (p.detach().double() - q.detach().double()).abs().cpu()
        bound = ours.Ep[i] + theirs.Ep[i] + (ours.P[i] - theirs.P[i]).abs() + TINY
        assert (d <= bound).all(), (i, (d / bound).max().item())
    # one group (or equal groups) keeps the fused backward
    m1, _ = _mlp_pair(gpu, seed=23)
    assert SGD(m1.parameters(), lr=lr, momentum=0.9, weight_decay=wd, fused_backward=True).fused_active()
    m2, _ = _mlp_pair(gpu, seed=23)
    o2 = SGD(_mlp_groups(m2, wd, lr), lr=lr, momentum=0.9, fused_backward=True, allow_groups=True)
    assert not o2.fused_active() and o2.flat.fused_opt is None


@pytest.mark.parametrize("clip", [None, 0.05], ids=["plain", "clipped"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_captured_two_group_step_replays_equal_eager_steps(gpu, kind, clip):
    """``tests/test_gpu_adamw.py``'s capture test with two groups: K = 5 replays of ONE captured step == 5 eager
    steps bit for bit in p, the states and the bf16 shadow."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import SGD, AdamW
    from ddpx.optim.schedule import one_cycle
    from ddpx.runtime.graphs import try_capture
    torch.manual_seed(5)
    a, b = MLP(hidden=512), MLP(hidden=512)
    b.load_state_dict(a.state_dict())
    opts = []
    for mdl in (a, b):
        ddpx.prepare_model(mdl, gpu)
        if kind == "sgd":
            o = SGD(_mlp_groups(mdl, 5e-4, 0.4), lr=0.4, momentum=0.9, capturable=True, fused_backward=True,
                    max_grad_norm=clip, allow_groups=True)
        else:
            o = AdamW(_mlp_groups(mdl, 0.01, 1e-3), lr=1e-3, betas=BETAS, eps=EPS, capturable=True, max_grad_norm=clip,
                      allow_groups=True)
        sched = one_cycle(o, 4, num_epochs=5)  # starts at lr = 0: the base rates define the multipliers
        assert o.attach_device_schedule(sched) and not o.fused_active() and not o._hyper().uniform
        assert min(o._hyper().lr_mul) == f32(0.1)
        opts.append(o)
    oa, ob = opts
    K = 5
    xs = [torch.rand(128, 3072, device=gpu).to(torch.bfloat16) for _ in range(K + 1)]
    ts = [torch.randint(0, 10, (128,), device=gpu) for _ in range(K + 1)]

    def body_of(model, opt):
        def body(x, y):
            opt.device_lr_step()
            opt.zero_grad()
            loss, _ = model.forward_loss(x, y)
            loss.backward()
            opt.step()
            return loss
        return body

    body_a, body_b = body_of(a, oa), body_of(b, ob)
    body_a(xs[0], ts[0])  # the trainer's eager warm-up step
    graph, err = try_capture(body_a, xs[1], ts[1], a, oa)
    assert graph is not None, err
    for i in range(1, K + 1):
        graph(xs[i], ts[i])
    for i in range(K + 1):
        body_b(xs[i], ts[i])
    torch.cuda.synchronize()
    fa, fb = oa.flat, ob.flat
    assert torch.equal(oa.lr_dev, ob.lr_dev) and oa.lr_dev.item() > 0
    assert torch.equal(fa.master, fb.master)
    for name in fa.state_tensors:
        assert torch.equal(fa.state_tensors[name], fb.state_tensors[name]), name
        assert fa.state_tensors[name].abs().sum().item() > 0
    assert torch.equal(fa.shadow, fb.shadow) and torch.equal(fa.shadow, fa.master.to(torch.bfloat16))
    if clip is not None:
        assert oa.grad_norm_dev.item() == ob.grad_norm_dev.item() > clip
