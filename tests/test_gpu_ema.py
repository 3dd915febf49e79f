"""``ddpx_ema_flat`` / ``ddpx_ema_advance`` (``csrc/kernels/ema.hip``) and ``ddpx.optim.WeightEMA`` on the GPU.

The kernel computes ``e = fma(p - e, w, e)``: two roundings.  Against ``ref = e + (p - e) * w`` in fp64 (with the
fp32 ``w``) that is at most ``u * w * |p - e|`` from rounding the difference plus ``u * |result|`` from the fma,
``u = 2^-24``; ``|result|`` is ``|ref|`` up to those errors, which the factor ``1 + 2^-20`` absorbs:

    |got - ref| <= 2^-24 * (w * |p - e| + |ref|) * (1 + 2^-20)

Over several steps an error already in the average is multiplied by ``1 - w`` by the next update, so the sum of the
per-step bounds bounds the error of the average against an fp64 replay from the same weights.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
DECAYS = [0.9, 0.999, 0.9999]


def _w_of(decay):
    from ddpx.ops.ema import ema_weight
    return ema_weight(1, 0, decay, False, 1)[1]


def _second_pass_size():
    """The smallest kind of size at which some threads of the capped grid run a second loop iteration with only ONE
    vector (T threads take 2 T vectors per iteration) and a 3-element scalar tail remains."""
    from ddpx.runtime import native
    T = native.kernels().ddpx_ema_max_threads()
    return 4 * (2 * T + 1000) + 3


def _data(n, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    e = torch.randn(n, generator=g)
    p = e + torch.randn(n, generator=g) * torch.logspace(-6, 0, n)
    return e.to(gpu), p.to(gpu)


def _bound(e0, p, ref, w):
    return U * (w * (p.double() - e0.double()).abs() + ref.abs()) * SLACK


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1031, "second-pass"])
def test_kernel_against_fp64_on_a_sub_range(gpu, n, decay):
    """Every size runs on a range that starts 4 (or 12) elements into a larger buffer; the elements before and after
    it keep their bits."""
    from ddpx.ops.ema import ema_flat_
    n = _second_pass_size() if n == "second-pass" else n
    assert n < 2 ** 23  # (16-20 MB)
    off, after = (4 if n % 2 else 12), 9
    e, p = _data(off + n + after, gpu, 11 + n % 97)
    e0 = e.clone()
    w = _w_of(decay)
    w_dev = torch.full((), w, dtype=torch.float32, device=gpu)
    assert w_dev.item() == w
    ema_flat_(e[off:off + n], p[off:off + n], w_dev)
    torch.cuda.synchronize()
    assert torch.equal(e[:off], e0[:off]) and torch.equal(e[off + n:], e0[off + n:])
    got, a, b = e[off:off + n], e0[off:off + n], p[off:off + n]
    ref = a.double() + (b.double() - a.double()) * w
    err, bound = (got.double() - ref).abs(), _bound(a, b, ref, w)
    worst = (err / bound).max().item()
    print(f"n={n} decay={decay}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), worst
    if n >= 1023:  # (the first elements' p - e is 1e-6 of e: w times it may round away)
        assert not torch.equal(got, a)
    # the host weight takes the same path bit for bit
    e2 = e0.clone()
    ema_flat_(e2[off:off + n], p[off:off + n], w)
    assert torch.equal(e2, e)


def test_zero_weight_returns_before_touching_anything(gpu):
    from ddpx.ops.ema import ema_flat_
    n = 4 * 1031 + 3
    e, p = _data(n, gpu, 5)
    p[::5] = float("inf")
    p[1::5] = float("nan")
    p[2::5] = float("-inf")
    e0 = e.clone()
    ema_flat_(e, p, torch.zeros((), dtype=torch.float32, device=gpu))
    ema_flat_(e, p, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(e, e0)


def test_refusals(gpu):
    from ddpx.runtime import native
    lib = native.kernels()
    e, p = _data(64, gpu, 6)
    e0 = e.clone()
    w = torch.full((), 0.5, dtype=torch.float32, device=gpu)
    s = native.stream_handle()
    assert lib.ddpx_ema_flat(e.data_ptr() + 4, p.data_ptr(), 32, w.data_ptr(), 0.0, s) != 0  # ema + 1
    assert lib.ddpx_ema_flat(e.data_ptr(), p.data_ptr() + 8, 32, w.data_ptr(), 0.0, s) != 0
    assert lib.ddpx_ema_flat(e.data_ptr(), p.data_ptr(), 32, w.data_ptr() + 2, 0.0, s) != 0
    assert lib.ddpx_ema_flat(None, p.data_ptr(), 32, None, 0.5, s) != 0
    assert lib.ddpx_ema_flat(e.data_ptr(), None, 32, None, 0.5, s) != 0
    assert lib.ddpx_ema_flat(e.data_ptr(), p.data_ptr(), 0, None, 0.5, s) == 0
    assert lib.ddpx_ema_flat(None, None, -3, None, 0.5, s) == 0
    c = torch.zeros(2, dtype=torch.int32, device=gpu)
    for decay, every in ((1.0, 1), (-0.1, 1), (float("nan"), 1), (0.9, 0)):
        assert lib.ddpx_ema_advance(c.data_ptr(), decay, 0, every, w.data_ptr(), s) != 0
    assert lib.ddpx_ema_advance(None, 0.9, 0, 1, w.data_ptr(), s) != 0
    torch.cuda.synchronize()
    assert torch.equal(e, e0) and c.tolist() == [0, 0] and w.item() == 0.5


@pytest.mark.parametrize("warmup,every", [(False, 1), (True, 1), (False, 3), (True, 3)])
def test_advance_kernel_against_its_host_twin(gpu, warmup, every):
    from ddpx.ops.ema import ema_advance_, ema_weight
    decay = 0.999
    c = torch.zeros(2, dtype=torch.int32, device=gpu)
    w = torch.full((), -1.0, dtype=torch.float32, device=gpu)
    u, seen = 0, []
    for s in range(1, 41):
        ema_advance_(c, decay, warmup, every, w)
        u, want = ema_weight(s, u, decay, warmup, every)
        got = w.item()
        assert c.tolist() == [s, u], (s, c.tolist())
        if every == 1 or want == 0.0:
            assert got == want, (s, got, want)
        else:  # device and host pow may differ in the last fp64 bit: at most the neighbouring fp32 value
            t = torch.tensor(want, dtype=torch.float32)
            lo, hi = torch.nextafter(t, t - 1).item(), torch.nextafter(t, t + 1).item()
            assert lo <= got <= hi, (s, got, want)
        seen.append(got)
    assert sum(1 for x in seen if x == 0.0) == (0 if every == 1 else 40 - 40 // 3)


def _make(kind, gpu, seed, with_ema):
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import SGD, AdamW, WeightEMA
    torch.manual_seed(seed)
    m = MLP(hidden=512)
    ddpx.prepare_model(m, gpu)
    if kind == "sgd":
        o = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
        assert o.fused_active()
    else:
        o = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=0.05)
    ema = WeightEMA(o, decay=0.9, every=1) if with_ema else None
    return m, o, ema


def _body_of(model, opt):
    def body(x, y):
        opt.zero_grad()
        loss, _ = model.forward_loss(x, y)
        loss.backward()
        opt.step()
        return loss
    return body


@pytest.mark.parametrize("kind", ["sgd-fused-backward", "adamw-clipped"])
def test_optimizer_steps_eager_then_captured(gpu, kind):
    """3 eager steps, then 3 replays of a captured step.  After every step the average is within the summed bound
    of an fp64 replay from the weights read back, the device counters count, and the training weights are the
    bits of the same run without an average."""
    from ddpx.ops.ema import ema_weight
    from ddpx.runtime.graphs import try_capture
    kind = kind.split("-")[0]
    m, o, ema = _make(kind, gpu, 3, True)
    m2, o2, _ = _make(kind, gpu, 3, False)
    assert torch.equal(o.flat.master, o2.flat.master) and torch.equal(ema.buffer, o.flat.master)
    assert ema.buffer is o.flat.state_tensors["ema"] and ema.counters_dev.tolist() == [0, 0]
    xs = [torch.rand(128, 3072, device=gpu).to(torch.bfloat16) for _ in range(6)]
    ts = [torch.randint(0, 10, (128,), device=gpu) for _ in range(6)]
    body, body2 = _body_of(m, o), _body_of(m2, o2)
    replay = ema.buffer.double()
    bound = torch.zeros_like(replay)
    graph = graph2 = None
    u = 0
    for k in range(6):
        if k == 3:
            graph, err = try_capture(body, xs[k], ts[k], m, o)
            assert graph is not None, err
            graph2, err = try_capture(body2, xs[k], ts[k], m2, o2)
            assert graph2 is not None, err
            assert ema.counters_dev.tolist() == [3, 3], "capturing must not run (or count) a step"
        if k < 3:
            body(xs[k], ts[k])
            body2(xs[k], ts[k])
        else:
            graph(xs[k], ts[k])
            graph2(xs[k], ts[k])
        torch.cuda.synchronize()
        u, w = ema_weight(k + 1, u, 0.9, False, 1)
        assert ema.weight_dev.item() == w
        p = o.flat.master.double()
        new = replay + (p - replay) * w
        bound += U * (w * (p - replay).abs() + new.abs()) * SLACK
        replay = new
        err = (ema.buffer.double() - replay).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{kind} step {k + 1}: max err / summed bound = {worst:.3f}")
        assert (err <= bound).all(), (k, worst)
        assert ema.counters_dev.tolist() == [k + 1, k + 1] and ema.counts() == (k + 1, k + 1)
        assert torch.equal(o.flat.master, o2.flat.master), k
        assert torch.equal(o.flat.shadow, o2.flat.shadow), k
    assert (ema.buffer - o.flat.master).abs().max().item() > 0
    if kind == "sgd":
        assert o.fused_active() and o.flat.fused_opt is o  # the fused backward stayed on


def test_every_3_updates_on_the_third_step_only(gpu):
    from ddpx.optim import WeightEMA
    m, o, _ = _make("adamw", gpu, 4, False)
    ema = WeightEMA(o, decay=0.9, every=3)
    body = _body_of(m, o)
    g = torch.Generator(device="cpu").manual_seed(0)
    for k in range(1, 4):
        before = ema.buffer.clone()
        body(torch.rand(128, 3072, generator=g).to(gpu).to(torch.bfloat16), torch.randint(0, 10, (128,)).to(gpu))
        torch.cuda.synchronize()
        assert torch.equal(ema.buffer, before) == (k < 3), k
    assert ema.counts() == (3, 1)


def test_applied_between_steps_changes_no_training_bit(gpu):
    """Two identical models; one enters and leaves ``applied()`` between steps 2 and 3."""
    from ddpx.train.checkpoint import model_state_dict
    a, oa, ea = _make("sgd", gpu, 9, True)
    b, ob, eb = _make("sgd", gpu, 9, True)
    xs = [torch.rand(128, 3072, device=gpu).to(torch.bfloat16) for _ in range(3)]
    ts = [torch.randint(0, 10, (128,), device=gpu) for _ in range(3)]
    ba, bb = _body_of(a, oa), _body_of(b, ob)
    for k in range(3):
        if k == 2:
            fa = oa.flat
            master, shadow, buf = fa.master.clone(), fa.shadow.clone(), ea.buffer.clone()
            want = ea.state_dict()["params"]
            with ea.applied():
                assert torch.equal(fa.master, buf) and torch.equal(fa.shadow, buf.to(torch.bfloat16))
                sd = model_state_dict(a)
                assert all(torch.equal(sd[n], v) for n, v in want.items())
            assert torch.equal(fa.master, master) and torch.equal(fa.shadow, shadow)
            assert torch.equal(ea.buffer, buf)
        ba(xs[k], ts[k])
        bb(xs[k], ts[k])
    torch.cuda.synchronize()
    assert torch.equal(oa.flat.master, ob.flat.master) and torch.equal(oa.flat.shadow, ob.flat.shadow)
    assert torch.equal(ea.buffer, eb.buffer) and torch.equal(oa.momentum_buffer, ob.momentum_buffer)


def test_state_dict_round_trip_restores_buffer_and_device_counters(gpu):
    a, oa, ea = _make("adamw", gpu, 2, True)
    body = _body_of(a, oa)
    for _ in range(2):
        body(torch.rand(128, 3072, device=gpu).to(torch.bfloat16), torch.randint(0, 10, (128,), device=gpu))
    sd = ea.state_dict()
    b, ob, eb = _make("adamw", gpu, 8, True)
    eb.load_state_dict(sd)
    assert eb.counters_dev.tolist() == [2, 2] == ea.counters_dev.tolist()
    for (n, p) in a.named_parameters():
        q = dict(b.named_parameters())[n]
        i, j = oa.flat.index[id(p)], ob.flat.index[id(q)]
        assert torch.equal(ea.buffer[oa.flat.slice(i)], eb.buffer[ob.flat.slice(j)]), n
