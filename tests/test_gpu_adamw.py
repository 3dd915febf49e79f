"""The fused flat AdamW on the GPU: ``ddpx_adamw_flat`` against fp64, ``ddpx.optim.AdamW`` against
``torch.optim.AdamW``, HIP-graph capture, clipping, a whole model and a full-checkpoint round trip.

Tolerances of one kernel step, counted from the sequence ``adamw_apply`` (``csrc/kernels/adamw.hip``) executes.
u = 2^-24 (one fp32 rounding multiplies its result by (1 + e), |e| <= u); first order in u.  The fp64 references
take the same fp32 inputs and the same fp32 scalars the kernel receives: lr, the two bias corrections the advance
kernel wrote, fp32(1 - beta1), fp32(beta2), fp32(1 - beta2), fp32(eps), fp32(wd) and the clip factor.

* m' = fma(g - m, w1, m), g = fl(g * gscale) when a scale applies.  Roundings: [g * gscale], g - m, the fma:
  K_M = 2 (+1).  Each is relative to a quantity bounded by |m| + |g|, so |m' - m^| <= K_M u (|m| + |g|), with g the
  scaled gradient (at most the unscaled one under a clip factor <= 1).
* v' = fma(beta2, v, fl(fl(g * g) * w2)).  Roundings: g * g, * w2, the fma: K_V = 3; a scaled g carries its own
  rounding into the square twice: +2.  Every term is >= 0, nothing cancels: |v' - v^| <= K_V u v^.
* p' = fma(p, decay, -upd) with decay = fma(-lr, wd, 1), upd = fl(fl(step * m') / denom), step = fl(lr / bc1),
  denom = fl(fl(sqrt(v') / bc2s) + eps).  Roundings: decay, lr / bc1, step * m', sqrt, / bc2s, + eps, / denom, the
  final fma: K_P = 8.  With p^ from the kernel's own m', v' (m's cancellation stays out):
  |p' - p^| <= u |p| (decay) + 6 u |upd| + u (|p| + |upd|) (final fma) <= K_P u (|p| + |upd|).

Every bound gets + 2^-149 (the smallest subnormal: an absolute rounding floor).  For orientation, torch's own fp32
CPU AdamW needs 0.99 / 2.74 / 4.35 of u against such references; the achieved constants are printed.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149
K_M, K_V, K_P = 2, 3, 8          # roundings of one kernel step, no gradient scale
K_M_SCALE, K_V_SCALE = 1, 2      # extra with a scale
# torch's fp32 GPU AdamW (its foreach op sequence, torch/optim/adam.py `_multi_tensor_adam`), counted the same way:
# m: lerp = sub + fma (2).  v: mul, g * g, * value, add (4).  p: fl(1 - lr*wd), p * decay; sqrt, / bc2s, + eps;
# m / denom, * step, add; step = fl64(lr / bc1) rounded once, against a reference built from fp32 lr and fp32 bc1
# (3): 12.  An in-place clip_grad_norm_ rounds the gradient once more (+1, +2).
T_M, T_V, T_P = 2, 4, 12
SWEEP = 2048 * 256 * 2 * 4  # elements of one full grid sweep: flat_grid_for's 2048 blocks x 256 x 2 vectors x 4
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)

SIZES = [1, 3, 4, 5, 63, 64, 65, 1023,
         SWEEP - 1, SWEEP, SWEEP + 1, SWEEP + 2, SWEEP + 3,       # around one sweep; n % 4 in {1, 2, 3} above it
         SWEEP + 4 * (SWEEP // 8 + 1000) + 2]                     # 2nd sweep: only 1000 threads get a second vector


def f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _inputs(n, gpu, gdtype, seed):
    """Non-trivial state (v >= 0); g == 0 on every 7th element, v == 0 on every 14th (so both on those), and
    m == 0 too on every 28th."""
    gen = torch.Generator(device=gpu).manual_seed(seed)
    p = torch.randn(n, device=gpu, generator=gen) * 0.1
    m = torch.randn(n, device=gpu, generator=gen) * 0.01
    v = (torch.randn(n, device=gpu, generator=gen) * 0.01).square()
    g = (torch.randn(n, device=gpu, generator=gen) * 0.02)
    g[::7] = 0
    v[::14] = 0
    m[::28] = 0
    return p, m, v, g.to(gdtype)


def _advance_to(t, gpu, betas):
    """(counter, bc) after the advance kernel took the counter from t - 1 to t."""
    from ddpx.ops.elementwise import adamw_advance_
    counter = torch.full((1,), t - 1, dtype=torch.int32, device=gpu)
    bc = torch.zeros(2, device=gpu)
    adamw_advance_(counter, bc, *betas)
    return counter, bc


def _check_step(p0, m0, v0, g, p1, m1, v1, lr, bc, clip, hp):
    """Elementwise check of one kernel step against fp64; returns the achieved constants (k_m, k_v, k_p)."""
    b1, b2 = hp["betas"]
    w1, b2f, w2 = f32(1.0 - b1), f32(b2), f32(1.0 - b2)
    eps, wd, lr = f32(hp["eps"]), f32(hp["weight_decay"]), f32(lr)
    bc1, bc2s = bc.double().tolist()
    scaled = clip is not None
    G = g.float().double() * (float(clip) if scaled else 1.0)
    P, M, V = p0.double(), m0.double(), v0.double()
    Mh = M + (G - M) * w1
    Vh = b2f * V + w2 * G * G
    Dn = v1.double().sqrt() / bc2s + eps
    Up = (lr / bc1) * m1.double() / Dn
    Ph = P * (1.0 - lr * wd) - Up
    for name, t in (("p", p1), ("m", m1), ("v", v1)):
        assert torch.isfinite(t).all(), f"{name}' has a non-finite element"
    km, kv = K_M + (K_M_SCALE if scaled else 0), K_V + (K_V_SCALE if scaled else 0)
    em = (m1.double() - Mh).abs()
    bm = U * (M.abs() + G.abs()) + TINY
    ev = (v1.double() - Vh).abs()
    bv = U * Vh + TINY
    ep = (p1.double() - Ph).abs()
    bp = U * (P.abs() + Up.abs()) + TINY
    got = ((em / bm).max().item(), (ev / bv).max().item(), (ep / bp).max().item())
    assert got[0] <= km, ("exp_avg", got, int((em / bm).argmax()))
    assert got[1] <= kv, ("exp_avg_sq", got, int((ev / bv).argmax()))
    assert got[2] <= K_P, ("param", got, int((ep / bp).argmax()))
    return got


def test_advance_kernel_counts_and_writes_both_corrections(gpu):
    b1, b2 = 0.9, 0.999
    for t in (1, 2, 3, 1000, 100000):
        counter, bc = _advance_to(t, gpu, (b1, b2))
        assert counter.item() == t
        want = [f32(1.0 - b1 ** t), f32(math.sqrt(1.0 - b2 ** t))]
        got = bc.tolist()
        # fp64 pow on the device against the host's: at most an fp64 ulp apart before the one fp32 rounding
        assert all(abs(a - b) <= U * b for a, b in zip(got, want)), (t, got, want)


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_step_matches_fp64(gpu, n, gdtype):
    """One step from given fp32 p, m, v, g for t in {1, 2, 1000}, with and without a clip scalar and the shadow;
    every element is compared (bounds: the module docstring)."""
    from ddpx.ops.elementwise import adamw_flat_
    worst = [0.0, 0.0, 0.0]
    for t in (1, 2, 1000):
        _, bc = _advance_to(t, gpu, HP["betas"])
        for use_clip in (False, True):
            for use_shadow in (False, True):
                p0, m0, v0, g = _inputs(n, gpu, gdtype, seed=n % 1000 + t)
                p, m, v = p0.clone(), m0.clone(), v0.clone()
                sh = torch.full((n,), float("nan"), dtype=torch.bfloat16, device=gpu) if use_shadow else None
                clip = torch.tensor(0.37, device=gpu) if use_clip else None
                # the learning rate from a device scalar in the clipped runs, from the host in the others
                lr = torch.tensor(HP["lr"], device=gpu) if use_clip else HP["lr"]
                adamw_flat_(p, m, v, g, sh, lr, bc, None, *HP["betas"], HP["eps"], HP["weight_decay"], clip=clip)
                got = _check_step(p0, m0, v0, g, p, m, v, HP["lr"], bc, clip, HP)
                worst = [max(a, b) for a, b in zip(worst, got)]
                if use_shadow:
                    assert torch.equal(sh.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
    print(f"n={n} {gdtype}: achieved k_m {worst[0]:.2f} k_v {worst[1]:.2f} k_p {worst[2]:.2f} "
          f"(bounds {K_M}+{K_M_SCALE} / {K_V}+{K_V_SCALE} / {K_P})")


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
@pytest.mark.parametrize("n", [1, 3, 1023, 4099])
def test_kernel_on_a_slice_leaves_its_neighbours_alone(gpu, n, gdtype):
    from ddpx.ops.elementwise import adamw_flat_
    tot = 64 + n + 64
    P0, M0, V0, G = _inputs(tot, gpu, gdtype, seed=5)
    P, M, V, G0 = P0.clone(), M0.clone(), V0.clone(), G.clone()
    S = torch.full((tot,), 3.0, dtype=torch.bfloat16, device=gpu)
    _, bc = _advance_to(2, gpu, HP["betas"])
    sl = slice(64, 64 + n)
    adamw_flat_(P[sl], M[sl], V[sl], G[sl], S[sl], HP["lr"], bc, None, *HP["betas"], HP["eps"], HP["weight_decay"])
    _check_step(P0[sl], M0[sl], V0[sl], G[sl], P[sl], M[sl], V[sl], HP["lr"], bc, None, HP)
    assert torch.equal(S[sl], P[sl].to(torch.bfloat16))
    for new, old in ((P, P0), (M, M0), (V, V0)):
        for outside in (slice(0, 64), slice(64 + n, tot)):
            assert torch.equal(new[outside].view(torch.int32), old[outside].view(torch.int32))
    assert torch.equal(G.view(torch.uint8), G0.view(torch.uint8))
    assert (S[:64] == 3).all() and (S[64 + n:] == 3).all()


def test_kernel_refuses_misaligned_buffers_and_ignores_empty_ones(gpu):
    from ddpx.ops.elementwise import adamw_flat_
    from ddpx.runtime.native import NativeError
    p, m, v, g = _inputs(64, gpu, torch.float32, seed=1)
    _, bc = _advance_to(1, gpu, HP["betas"])
    args = (HP["lr"], bc, None, *HP["betas"], HP["eps"], HP["weight_decay"])
    with pytest.raises(NativeError):
        adamw_flat_(p[1:33], m[:32], v[:32], g[:32], None, *args)
    with pytest.raises(NativeError):
        adamw_flat_(p[:32], m[:32], v[2:34], g[:32], None, *args)
    before = p.clone()
    adamw_flat_(p[:0], m[:0], v[:0], g[:0], None, *args)
    assert torch.equal(p, before)


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
def test_sweep_coverage_every_element_written(gpu, gdtype):
    """Inputs chosen so that every output element must differ from its input (g in [1.5, 2.5), m in [0.25, 0.75):
    m moves towards g by a tenth of at least 0.75; v ~ 1e-4 gains 1e-3 g^2; p ~ 1 moves by ~1e-3): an element
    the sweep skipped keeps its input bits and shows up by itself, not in a norm."""
    from ddpx.ops.elementwise import adamw_flat_
    n = SIZES[-1]
    gen = torch.Generator(device=gpu).manual_seed(9)
    r = [torch.rand(n, device=gpu, generator=gen) + 0.5 for _ in range(4)]
    p0, m0, v0, g = r[0], r[1] * 0.5, r[2] * 1e-4, (r[3] + 1.0).to(gdtype)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    sh = torch.full((n,), float("nan"), dtype=torch.bfloat16, device=gpu)
    _, bc = _advance_to(3, gpu, HP["betas"])
    adamw_flat_(p, m, v, g, sh, HP["lr"], bc, None, *HP["betas"], HP["eps"], HP["weight_decay"])
    for name, new, old in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
        same = (new == old).nonzero()
        assert same.numel() == 0, (name, "unwritten from", int(same[0]), "count", same.numel())
    assert not torch.isnan(sh.float()).any()
    assert torch.equal(sh, p.to(torch.bfloat16))
    _check_step(p0, m0, v0, g, p, m, v, HP["lr"], bc, None, HP)


# ----------------------------------------------------------------------------------------------- the optimizer
class _Odd(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n) * 0.1) for n in sizes])


ODD = [1, 3, 4, 63, 64, 65, 1023, 4099, 70001]


def _fill(flat, seed, scale=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat.grad.fill_(float("nan"))  # the padding stays NaN: it must never be read into a parameter
    for p in flat.params:
        x = torch.randn(p.shape, generator=g) * scale
        x.view(-1)[::5] = 0
        p.main_grad.copy_(x.to(flat.device))
        flat.grad_done(p)


def _twins(gpu, seed, shadow=False):
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m = _Odd(ODD).to(gpu)
    twin = _Odd(ODD).to(gpu)
    twin.load_state_dict(m.state_dict())
    return m, twin, FlatParams(m, shadow_dtype=torch.bfloat16 if shadow else None)


def _same_bits(fa, fb, pairs):
    """Every parameter's slice of each (tensor of store a, tensor of store b) pair holds the same bits (the
    padding between parameters is nobody's: it took the NaN of the gradient padding)."""
    for i in range(len(fa.params)):
        sa, sb = fa.slice(i), fb.slice(fb.index[id(fb.params[i])])
        for k, (ta, tb) in enumerate(pairs):
            assert torch.equal(ta[sa], tb[sb]), (i, k)


class _Fp64Run:
    """The same steps in fp64 from the same fp32 gradients and fp32 scalars, and next to it the first-order
    bounds on an fp32 implementation's distance from it, accumulated over the steps, per unit of its per-step
    rounding counts (k_m, k_v, k_p) — linear in them, so two implementations are at most the sum of their
    bounds apart:

      E_m <- (1 - w1) E_m + k_m u (|m| + |g|) + w1 eg |g|        an old error decays with the average
      R_v <- R_v + k_v u + 2 eg                                  relative; all terms >= 0
      E_u  = step E_m / denom + |upd| R_v / 2                    sqrt halves v's relative error; eps only helps
      E_p <- E_p + E_u + k_p u (|p| + |upd|)                     the decay factor <= 1 does not amplify E_p

    ``eg``: relative distance between the gradient scales of the two runs (the clip factors)."""

    def __init__(self, params, hp, k, eg=0.0):
        self.P = [p.detach().double().clone() for p in params]
        self.M = [torch.zeros_like(p) for p in self.P]
        self.V = [torch.zeros_like(p) for p in self.P]
        self.Em = [torch.zeros_like(p) for p in self.P]
        self.Rv = 0.0
        self.Ep = [torch.zeros_like(p) for p in self.P]
        self.hp, self.k, self.eg = hp, k, eg

    def step(self, grads, lr, bc, gscale=1.0):
        b1, b2 = self.hp["betas"]
        w1, b2f, w2 = f32(1.0 - b1), f32(b2), f32(1.0 - b2)
        eps, wd, lr = f32(self.hp["eps"]), f32(self.hp["weight_decay"]), f32(lr)
        bc1, bc2s = bc
        km, kv, kp = self.k
        self.Rv += kv * U + 2 * self.eg
        for i, g in enumerate(grads):
            G = g.double() * gscale
            self.Em[i] = (1 - w1) * self.Em[i] + km * U * (self.M[i].abs() + G.abs()) + w1 * self.eg * G.abs()
            self.M[i] = self.M[i] + (G - self.M[i]) * w1
            self.V[i] = b2f * self.V[i] + w2 * G * G
            dn = self.V[i].sqrt() / bc2s + eps
            up = (lr / bc1) * self.M[i] / dn
            self.Ep[i] = (self.Ep[i] + (lr / bc1) * self.Em[i] / dn + up.abs() * self.Rv / 2
                          + kp * U * (self.P[i].abs() + up.abs()))
            self.P[i] = self.P[i] * (1.0 - lr * wd) - up

    def bounds(self, i):
        return self.Em[i] + TINY, self.Rv * self.V[i] + TINY, self.Ep[i] + TINY


def _compare_runs(opt, topt, m, twin, ref, label):
    """ours vs torch within the summed bounds (``ref`` was built with k = ours + torch's); prints each side's own
    distance from the fp64 run in units of the unit-k bound."""
    sd = opt.state_dict()["state"]
    ku = [a + b for a, b in zip((K_M, K_V, K_P), (T_M, T_V, T_P))]
    worst_o, worst_t, worst_d = [0.0] * 3, [0.0] * 3, [0.0] * 3
    for i, (p, q) in enumerate(zip(m.parameters(), twin.parameters())):
        st = topt.state[q]
        trip_o = (sd[i]["exp_avg"], sd[i]["exp_avg_sq"], p.detach())
        trip_t = (st["exp_avg"], st["exp_avg_sq"], q.detach())
        trip_r = (ref.M[i], ref.V[i], ref.P[i])
        for j, (a, b, r, bound) in enumerate(zip(trip_o, trip_t, trip_r, ref.bounds(i))):
            assert torch.isfinite(a).all()
            d = (a.double() - b.double()).abs()
            assert (d <= bound).all(), (label, i, "mvp"[j], (d / bound).max().item())
            worst_d[j] = max(worst_d[j], (d / bound).max().item())
            # per unit k: the summed-k bound scaled back (the eg terms make this an upper estimate of the unit)
            unit = bound / ku[j]
            worst_o[j] = max(worst_o[j], ((a.double() - r).abs() / unit).max().item())
            worst_t[j] = max(worst_t[j], ((b.double() - r).abs() / unit).max().item())
    print(f"{label}: |ours - torch| / bound (m, v, p) = {[round(x, 3) for x in worst_d]}; distance from the fp64 "
          f"run in unit-k bounds: ours {[round(x, 2) for x in worst_o]} torch {[round(x, 2) for x in worst_t]}")


def test_five_eager_steps_match_torch_adamw(gpu):
    """``ddpx.optim.AdamW`` (eager, host LR, device step counter) against ``torch.optim.AdamW`` on the GPU from the
    same init and gradients.  Bound: ``_Fp64Run``'s accumulation with k = the kernel's counts + torch's."""
    from ddpx.optim import AdamW
    m, twin, flat = _twins(gpu, seed=11)
    opt = AdamW(m.parameters(), **HP)
    topt = torch.optim.AdamW(twin.parameters(), **HP)
    ref = _Fp64Run(list(m.parameters()), HP, (K_M + T_M, K_V + T_V, K_P + T_P))
    for step in range(5):
        opt.zero_grad()
        _fill(flat, 20 + step, scale=1e-5 if step == 2 else 0.02)
        grads = [p.main_grad.detach().clone() for p in m.parameters()]
        for q, g in zip(twin.parameters(), grads):
            q.grad = g.clone()
        opt.step()
        topt.step()
        ref.step(grads, HP["lr"], opt._bc_dev.double().tolist())
    assert opt.steps_taken() == 5 and opt.step_dev.item() == 5 and flat.fused_opt is None
    _compare_runs(opt, topt, m, twin, ref, "5 eager steps")


@pytest.mark.parametrize("max_norm", [1e9, 0.05])
def test_clipped_steps(gpu, max_norm):
    """A bound so large that the factor is exactly 1.0: the bits of the unclipped optimizer.  A small bound:
    ``clip_grad_norm_`` + ``torch.optim.AdamW`` within the accumulated bounds, the two clip factors apart by
    ``tests/test_gpu_clip.py``'s BOUND on the norm (+ 4 u: torch's norm, + 1e-6, the division, ours likewise)."""
    from ddpx.optim import AdamW
    from tests.test_gpu_clip import BOUND
    m, twin, flat = _twins(gpu, seed=12)
    opt = AdamW(m.parameters(), max_grad_norm=max_norm, **HP)
    if max_norm > 1:
        plain_m, _, plain_flat = _twins(gpu, seed=12)
        plain = AdamW(plain_m.parameters(), **HP)
    topt = torch.optim.AdamW(twin.parameters(), **HP)
    eg = 2 * BOUND + 4 * U
    ref = _Fp64Run(list(m.parameters()), HP, (K_M + K_M_SCALE + T_M + 1, K_V + K_V_SCALE + T_V + 2, K_P + T_P), eg)
    for step in range(3):
        opt.zero_grad()
        _fill(flat, 30 + step)
        grads = [p.main_grad.detach().clone() for p in m.parameters()]
        for q, g in zip(twin.parameters(), grads):
            q.grad = g.clone()
        opt.step()
        tn = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
        topt.step()
        assert abs(opt.grad_norm_dev.item() - tn.item()) <= BOUND * tn.item()
        coef = opt.clip_coef_dev.item()
        if max_norm > 1:
            assert coef == 1.0
            plain.zero_grad()
            _fill(plain_flat, 30 + step)
            plain.step()
        else:
            assert tn.item() > 2 * max_norm and coef < 0.5, "the clip must be active"
        ref.step(grads, HP["lr"], opt._bc_dev.double().tolist(), gscale=coef)
    if max_norm > 1:
        _same_bits(flat, plain_flat, [(flat.master, plain_flat.master), (opt.exp_avg, plain.exp_avg),
                                      (opt.exp_avg_sq, plain.exp_avg_sq)])
    _compare_runs(opt, topt, m, twin, ref, f"3 clipped steps (max_norm {max_norm})")


@pytest.mark.parametrize("clip", [None, 0.05], ids=["plain", "clipped"])
def test_captured_step_replays_equal_eager_steps(gpu, clip):
    """The training step captured as the trainer captures it (``capturable=True``, device LR table attached):
    K = 5 replays of ONE captured step == 5 eager steps bit for bit in p, both states, the bf16 shadow and the
    device step counter; between replays the host writes nothing but the next batch."""
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import AdamW
    from ddpx.optim.schedule import one_cycle
    from ddpx.runtime.graphs import try_capture
    torch.manual_seed(5)
    a, b = MLP(hidden=256), MLP(hidden=256)
    b.load_state_dict(a.state_dict())
    opts = []
    for mdl in (a, b):
        ddpx.prepare_model(mdl, gpu)
        o = AdamW(mdl.parameters(), capturable=True, max_grad_norm=clip, **HP)
        sched = one_cycle(o, 4, num_epochs=5)  # a short cycle: the LR moves visibly on every step
        assert o.attach_device_schedule(sched)
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
    assert oa.step_dev.item() == 1, "capturing must not run (or count) a step"
    for i in range(1, K + 1):
        graph(xs[i], ts[i])
    for i in range(K + 1):
        body_b(xs[i], ts[i])
    torch.cuda.synchronize()
    fa, fb = oa.flat, ob.flat
    assert oa.step_dev.item() == ob.step_dev.item() == K + 1
    assert torch.equal(oa._bc_dev, ob._bc_dev) and torch.equal(oa.lr_dev, ob.lr_dev)
    assert torch.equal(fa.master, fb.master)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    assert torch.equal(fa.shadow, fb.shadow) and torch.equal(fa.shadow, fa.master.to(torch.bfloat16))
    assert oa.exp_avg_sq.abs().sum().item() > 0 and fa.fused_opt is None
    if clip is not None:
        assert oa.grad_norm_dev.item() == ob.grad_norm_dev.item() > clip


def test_whole_model_tracks_a_torch_fp32_twin(gpu):
    """``--model mlp --hidden 256 --batch_size 128 --dtype bf16 --optimizer adamw`` built as the training scripts
    build it, 6 steps on one batch against a torch fp32 twin with ``torch.optim.AdamW`` from the same init, within
    the tolerance ``smoke()`` uses for its SGD twin (3 % + 0.02 on every loss)."""
    from ddpx.models import MLP
    from ddpx.optim import AdamW
    from ddpx.train.app import build_model_and_optimizer, build_parser
    torch.manual_seed(0)
    args = build_parser("t").parse_args(["1", "1", "--model", "mlp", "--hidden", "256", "--batch_size", "128",
                                         "--dtype", "bf16", "--kernels", "native", "--optimizer", "adamw"])
    model, opt = build_model_and_optimizer(args, gpu)
    assert type(opt) is AdamW and model.use_native and opt.flat.fused_opt is None and not opt.fused_active()
    twin = MLP(hidden=256, layers=3)
    twin.load_state_dict(model.state_dict())
    twin = twin.to(gpu)
    twin.use_native = False
    twin.compute_dtype = torch.float32
    topt = torch.optim.AdamW(twin.parameters(), lr=args.lr, betas=tuple(args.betas), eps=args.eps,
                             weight_decay=args.weight_decay)
    x = torch.rand(128, 3072, device=gpu).to(torch.bfloat16)
    y = torch.randint(0, 10, (128,), device=gpu)
    losses, ref = [], []
    for _ in range(6):
        opt.zero_grad()
        loss, _ = model.forward_loss(x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        topt.zero_grad()
        tl = torch.nn.functional.cross_entropy(twin(x.float()), y)
        tl.backward()
        topt.step()
        ref.append(float(tl.item()))
    print("adamw losses", losses, "torch fp32 twin", ref)
    assert all(math.isfinite(v) for v in losses), losses
    for a, b in zip(losses, ref):
        assert abs(a - b) <= 0.03 * abs(b) + 0.02, (losses, ref)
    assert losses[-1] < losses[0], losses
    assert opt.step_dev.item() == 6


def test_full_checkpoint_round_trip(gpu, tmp_path):
    """3 steps, save, continue in a fresh model + optimizer loaded from the file: the next 2 steps are bitwise the
    uninterrupted run's (weights, both states, shadow, step count)."""
    from ddpx.optim import AdamW
    from ddpx.train.checkpoint import load_full_checkpoint, save_full_checkpoint
    path = str(tmp_path / "full.pt")
    m, _, flat = _twins(gpu, seed=13, shadow=True)
    opt = AdamW(m.parameters(), **HP)
    for step in range(5):
        if step == 3:
            save_full_checkpoint(path, m, opt, None, epoch=0)
        opt.zero_grad()
        _fill(flat, 40 + step)
        opt.step()
    m2, _, flat2 = _twins(gpu, seed=99, shadow=True)  # another init: everything must come from the file
    opt2 = AdamW(m2.parameters(), lr=0.5, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5)
    assert load_full_checkpoint(path, m2, opt2, None, map_location=gpu) == 1
    assert opt2.step_dev.item() == 3 and opt2.param_groups[0]["lr"] == HP["lr"]
    for step in (3, 4):
        opt2.zero_grad()
        _fill(flat2, 40 + step)
        opt2.step()
    assert opt2.steps_taken() == 5
    _same_bits(flat, flat2, [(flat.master, flat2.master), (flat.shadow, flat2.shadow), (opt.exp_avg, opt2.exp_avg),
                             (opt.exp_avg_sq, opt2.exp_avg_sq)])
    # the other optimizer's file is refused
    from ddpx.optim import SGD
    m3, _, _ = _twins(gpu, seed=1)
    with pytest.raises(ValueError, match="another optimizer"):
        load_full_checkpoint(path, m3, SGD(m3.parameters(), lr=0.1, momentum=0.9), None, map_location=gpu)
