"""The classifier head for 11..128 classes on the GPU (``csrc/kernels/head_xent.hip`` and the class-block kernels
of ``f32_head.hip``): element-exact logits and gradients on integer operands, loss / dlogits against fp64 with the
bars of ``test_gpu_soft_targets.py``, the n*u accuracy bound of the exact-f32 backward, the fused SGD against the
stored backward + ``sgd_flat_``, and repeatability.

``h`` is a :func:`tests._exact.poisoned` view (leading dimension K + 8, NaN padding).  The kernels take ``w``
contiguous, so its poison is a NaN-filled flat buffer that holds the [C, K] block 8 elements in: a read before the
first or past the last row shows as a NaN."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

pytestmark = pytest.mark.gpu


def _w_poisoned(t, gpu):
    C, K = t.shape
    buf = torch.full((C * K + 16,), float("nan"), dtype=torch.bfloat16, device=gpu)
    w = buf[8:8 + C * K].view(C, K)
    w.copy_(t.to(torch.bfloat16))
    return w


def _first_argmax(z):
    C = z.shape[1]
    ismax = z == z.max(1, keepdim=True).values
    return torch.where(ismax, torch.arange(C)[None, :], torch.full((1, 1), C)).min(1).values


@functools.lru_cache(maxsize=None)
def _fwd_case(C, M, K):
    s = 10007 * C + 101 * M + K
    h, w, b = X.ints((M, K), -2, 2, s), X.ints((C, K), -1, 1, s + 1), X.ints((C,), -4, 4, s + 2)
    t = torch.randint(0, C, (M,), generator=torch.Generator().manual_seed(s + 3))
    ref = h @ w.t() + b
    return h, w, b, t, ref, int((_first_argmax(ref) == t).sum())


# ------------------------------------------------------------------ 1. exact forward
@pytest.mark.parametrize("K", [32, 160, 512])
@pytest.mark.parametrize("M", [1, 16, 17, 50])
@pytest.mark.parametrize("C", [17, 32, 100, 128])
def test_forward_exact_bf16(gpu, C, M, K):
    from ddpx.ops.head import head_forward
    X.require_exact(2, 1, K + 4, "head forward")  # K products of at most 2, plus the bias
    h, w, b, t, ref, nhit = _fwd_case(C, M, K)
    hits = torch.zeros((), dtype=torch.int32, device=gpu)
    loss, logits, dl = head_forward(X.poisoned(h, gpu), _w_poisoned(w, gpu), b.float().to(gpu), t.to(gpu),
                                    correct=hits)
    X.assert_equal(logits, ref.float(), f"wide head logits C={C} M={M} K={K}")
    assert hits.item() == nhit  # ties are frequent on integer logits: the first maximum counts
    assert torch.isfinite(loss).item() and torch.isfinite(dl).all().item()
    # logits only, and a launch that wants neither logits nor gradient
    _, only, none = head_forward(X.poisoned(h, gpu), _w_poisoned(w, gpu), b.float().to(gpu))
    X.assert_equal(only, ref.float(), "logits only")
    assert none is None
    loss2, no_logits, no_dl = head_forward(X.poisoned(h, gpu), _w_poisoned(w, gpu), b.float().to(gpu), t.to(gpu),
                                           want_logits=False, want_grad=False)
    assert no_logits is None and no_dl is None and torch.equal(loss2, loss)


@pytest.mark.parametrize("K", [32, 160, 512])
@pytest.mark.parametrize("M", [1, 16, 17, 50])
@pytest.mark.parametrize("C", [17, 32, 100, 128])
def test_forward_exact_fp32(gpu, C, M, K):
    from ddpx.ops import f32
    from ddpx.ops.head import accuracy_count
    X.require_exact(2, 1, K + 4, "fp32 head forward")
    h, w, b, t, ref, nhit = _fwd_case(C, M, K)
    loss, logits, dl = f32.head_forward(h.float().to(gpu), w.float().to(gpu), b.float().to(gpu), t.to(gpu))
    X.assert_equal(logits, ref.float(), f"fp32 head logits C={C} M={M} K={K}")
    hits = torch.zeros((), dtype=torch.int32, device=gpu)
    accuracy_count(logits, t.to(gpu), hits)
    assert hits.item() == nhit
    assert torch.isfinite(loss).item() and torch.isfinite(dl).all().item()


# ------------------------------------------------------------------ 2. loss and dlogits
def _real_inputs(gpu, C, M, K, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(M, K, generator=g)).to(dtype).to(gpu)
    w = (torch.randn(C, K, generator=g) * (2.0 / K ** 0.5)).to(dtype).to(gpu)
    b = (torch.randn(C, generator=g) * 0.1).to(gpu)
    a = torch.randint(0, C, (M,), generator=g).to(gpu)
    tb = torch.randint(0, C, (M,), generator=g).to(gpu)
    lam = torch.rand(M, generator=g)
    lam[0], lam[1], lam[2] = 0.0, 1.0, 0.5
    return h, w, b, a, tb, lam.to(gpu)


def _hard_err(head_forward, gpu, C, M, K, dtype):
    """max |dlogits - fp64| of the hard launch on the kernel's own logits."""
    h, w, b, a, _, _ = _real_inputs(gpu, C, M, K, 11 * M + K, dtype)
    _, logits, dl = head_forward(h, w, b, a)
    p = torch.softmax(logits.double(), 1)
    return (dl.double() - (p - F.one_hot(a, C).double()) / M).abs().max().item()


def _check_loss(head_forward, gpu, C, M, K, eps, dtype, loss_tol):
    from ddpx.ops.loss import SoftTargets
    h, w, b, a, tb, lam = _real_inputs(gpu, C, M, K, 11 * M + K, dtype)
    bf = dtype == torch.bfloat16
    hits = torch.zeros((), dtype=torch.int32, device=gpu)
    kw = {"correct": hits} if bf else {}
    loss, logits, dl = head_forward(h, w, b, a, soft=SoftTargets(tb, lam, eps), **kw)
    hard_loss, hard_logits, hard_dl = head_forward(h, w, b, a)
    assert torch.equal(logits, hard_logits)
    z = logits.double()
    q = lam.double()[:, None] * F.one_hot(a, C).double() + (1 - lam.double()[:, None]) * F.one_hot(tb, C).double()
    qs = (1 - eps) * q + eps / C
    ref = F.cross_entropy(z, q, label_smoothing=eps).item()
    ref_hard = F.cross_entropy(z, a).item()
    p = torch.softmax(z, 1)
    err_hard = (hard_dl.double() - (p - F.one_hot(a, C).double()) / M).abs().max().item()
    err_soft = (dl.double() - (p - qs) / M).abs().max().item()
    err10 = _hard_err(head_forward, gpu, 10, M, K, dtype)  # today's 10-class kernel, same distribution, M, K
    bound = 2 * err_hard + 8 * 2.0 ** -24 / M
    print(f"head {dtype} C={C} M={M} K={K} eps={eps}: loss err soft {abs(loss.item() - ref):.3e} hard "
          f"{abs(hard_loss.item() - ref_hard):.3e} (tol {loss_tol(ref):.1e}); dlogits err hard {err_hard:.3e} "
          f"(C=10 kernel {err10:.3e}, bar {2 * err10:.3e}), soft {err_soft:.3e} (bar {bound:.3e})")
    assert abs(loss.item() - ref) < loss_tol(ref)
    assert abs(hard_loss.item() - ref_hard) < loss_tol(ref_hard)
    assert err_hard <= 2 * err10
    assert err_soft <= bound
    if bf:
        assert hits.item() == (_first_argmax(logits.cpu()) == a.cpu()).sum().item()
    # degenerate soft targets: the hard launch's bits
    for soft in (SoftTargets(tb, torch.ones_like(lam), 0.0), SoftTargets(None, None, 0.0), SoftTargets(None, lam, 0.0)):
        got = head_forward(h, w, b, a, soft=soft)
        for x, y in zip(got, (hard_loss, hard_logits, hard_dl)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [16, 17, 48])
@pytest.mark.parametrize("C", [17, 100])
def test_loss_dlogits_bf16(gpu, C, M, K, eps):
    from ddpx.ops.head import head_forward
    _check_loss(head_forward, gpu, C, M, K, eps, torch.bfloat16, lambda ref: 1e-4 * max(1.0, abs(ref)))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [16, 17, 48])
@pytest.mark.parametrize("C", [17, 100])
def test_loss_dlogits_fp32(gpu, C, M, K, eps):
    from ddpx.ops import f32
    _check_loss(f32.head_forward, gpu, C, M, K, eps, torch.float32, lambda ref: 1e-5)


def test_lr_advance_at_100_classes(gpu):
    from ddpx.ops.head import head_forward
    from ddpx.ops.loss import SoftTargets
    h, w, b, a, tb, lam = _real_inputs(gpu, 100, 48, 256, 5, torch.bfloat16)
    table = torch.tensor([0.5, 0.25, 0.125], device=gpu)
    state = {}
    for name, soft in (("hard", None), ("soft", SoftTargets(tb, lam, 0.1))):
        counter = torch.zeros(1, dtype=torch.int32, device=gpu)
        lr = torch.zeros(1, device=gpu)
        seen = []
        for _ in range(5):  # runs off the table's end: the last entry holds
            kw = {"soft": soft} if soft is not None else {}
            head_forward(h, w, b, a, lr_advance=(table, counter, lr), **kw)
            seen.append((counter.item(), lr.item()))
        state[name] = seen
    assert state["hard"] == [(1, 0.5), (2, 0.25), (3, 0.125), (4, 0.125), (5, 0.125)]
    assert state["soft"] == state["hard"]


# ------------------------------------------------------------------ 3. exact backward
@functools.lru_cache(maxsize=None)
def _bwd_case(C, M, K):
    s = 7919 * C + 31 * M + K
    dl = X.ints((M, C), -3, 3, s)
    h, mask = X.mask_operand((M, K), s + 1)
    w = X.ints((C, K), -2, 2, s + 2)
    return dl, h, mask, w, dl.t() @ h.double(), dl.sum(0), dl @ w


def _guard1(n, dtype, gpu):
    buf = torch.full((n + 16,), X.SENTINEL[dtype], dtype=dtype, device=gpu)
    return buf, buf[8:8 + n]


@pytest.mark.parametrize("K", [32, 160])
@pytest.mark.parametrize("M", [7, 50, 300])
@pytest.mark.parametrize("C", [12, 17, 100, 128])
def test_backward_exact(gpu, C, M, K):
    from ddpx.ops.head import head_backward
    # |go dl h| <= 0.5 * 3 * 3 in steps of 1/4 over M rows; |go dl w| <= 6 in steps of 1/2 over C classes, times 2
    X.require_exact(4 * 3, 3, M, "head dW")
    X.require_exact(2 * 3, 2 * 2, C, "head dH")
    dl, h, mask, w, dw64, db64, g64 = _bwd_case(C, M, K)
    dl_d = dl.float().to(gpu)
    variants = [(go, hs, rm, torch.float32, False) for go in (1.0, 0.5) for hs in (1.0, 2.0) for rm in (True, False)]
    variants += [(0.5, 2.0, True, torch.float32, True), (1.0, 1.0, True, torch.bfloat16, False),
                 (0.5, 1.0, False, torch.bfloat16, True)]
    for go, hs, rm, gdt, acc in variants:
        what = f"C={C} M={M} K={K} go={go} hscale={hs} relu_mask={rm} {gdt} accumulate={acc}"
        h_d, w_d = X.poisoned(h, gpu), _w_poisoned(w, gpu)
        wbuf, dW = X.guarded(C, K, gdt, gpu, ldc=K)
        hbuf, dH = X.guarded(M, K, torch.bfloat16, gpu)
        bbuf, db = _guard1(C, gdt, gpu)
        pbuf, dbp = _guard1(K, gdt, gpu)
        old = [torch.zeros(C, K, dtype=torch.float64), torch.zeros(C, dtype=torch.float64),
               torch.zeros(K, dtype=torch.float64)]
        if acc:
            old = [X.ints((C, K), -2, 2, 5), X.ints((C,), -2, 2, 6), X.ints((K,), -2, 2, 7)]
            for dst, o in zip((dW, db, dbp), old):
                dst.copy_(o.to(gdt))
        head_backward(dl_d, torch.tensor(go, device=gpu), h_d, w_d, dW, db, dH=dH, dbprev=dbp, relu_mask=rm,
                      accumulate=acc, dh_scale=hs)
        dh_ref = X.rounded(hs * (go * g64 * mask if rm else go * g64), torch.bfloat16)
        X.assert_equal(dH, dh_ref, "dH " + what)
        X.assert_equal(dW, X.rounded(go * dw64 + old[0], gdt), "dW " + what)
        X.assert_equal(db, X.rounded(go * db64 + old[1], gdt), "db " + what)
        X.assert_equal(dbp, X.rounded(dh_ref.double().sum(0) + old[2], gdt), "dbprev " + what)
        X.assert_guard(wbuf, C, K, "dW " + what)
        X.assert_guard(hbuf, M, K, "dH " + what)
        X.assert_guard_1d(bbuf, 8, 8 + C, "db " + what)
        X.assert_guard_1d(pbuf, 8, 8 + K, "dbprev " + what)


# ------------------------------------------------------------------ 4. accuracy of the backward
def test_backward_accuracy(gpu):
    """n*u bound of fp32 accumulation in any order, doubled for the MFMA's internal rounding; dlogits rounded to
    bf16 (relative error 2^-9 per term) would miss it by orders of magnitude."""
    from ddpx.ops.head import head_backward
    C, M, K, go, hs = 100, 300, 160, 0.5, 2.0
    g = torch.Generator().manual_seed(17)
    dl = torch.randn(M, C, generator=g) / M
    h = torch.relu(torch.randn(M, K, generator=g)).to(torch.bfloat16)
    w = (torch.randn(C, K, generator=g) * (2.0 / K ** 0.5)).to(torch.bfloat16)
    dW = torch.empty(C, K, device=gpu)
    db, dbp = torch.empty(C, device=gpu), torch.empty(K, device=gpu)
    dH = torch.empty(M, K, dtype=torch.bfloat16, device=gpu)
    head_backward(dl.to(gpu), torch.tensor(go, device=gpu), h.to(gpu), w.to(gpu), dW, db, dH=dH, dbprev=dbp,
                  relu_mask=True, dh_scale=hs)
    u = 2.0 ** -24
    dl64, h64, w64 = dl.double(), h.double(), w.double()
    dw_ref = go * dl64.t() @ h64
    dw_bound = 2 * (M + 8) * u * (go * dl64.abs().t() @ h64.abs())
    dw_err = (dW.cpu().double() - dw_ref).abs()
    mask = (h64 > 0).double()
    dh_ref = hs * mask * (go * dl64 @ w64)
    dh_bound = 2.0 ** -8 * dh_ref.abs() + 2 * (C + 8) * u * hs * (go * dl64.abs() @ w64.abs())
    dh_err = (dH.cpu().double() - dh_ref).abs()
    print(f"wide backward accuracy: dW err / bound max {(dw_err / dw_bound.clamp_min(1e-300)).max().item():.3f}, "
          f"dH err / bound max {(dh_err / dh_bound.clamp_min(1e-300)).max().item():.3f}")
    assert (dw_err <= dw_bound).all()
    assert (dh_err <= dh_bound).all()


# ------------------------------------------------------------------ 5. fused SGD
@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_backward_fused_sgd(gpu, mom):
    from ddpx.ops.elementwise import sgd_flat_
    from ddpx.ops.head import head_backward
    C, M, K, wd = 100, 50, 160, 5e-4
    g = torch.Generator().manual_seed(23)
    dl = (torch.randn(M, C, generator=g) / M).to(gpu)
    h = torch.relu(torch.randn(M, K, generator=g)).to(torch.bfloat16).to(gpu)
    lr = torch.tensor(0.1, device=gpu)
    go = torch.tensor(1.0, device=gpu)
    masters = [(torch.randn(C, K, generator=g) * 0.1).to(gpu), (torch.randn(C, generator=g) * 0.1).to(gpu),
               (torch.randn(K, generator=g) * 0.1).to(gpu)]
    bufs = [(torch.randn(m.shape, generator=g) * 0.01).to(gpu) for m in masters]

    def state():
        ms = [m.clone() for m in masters]
        return ms, [b.clone() for b in bufs], [m.to(torch.bfloat16) for m in ms]

    # stored backward, then the flat SGD kernel on the same buffers
    ms, bs, sh = state()
    dW, db, dbp = torch.empty(C, K, device=gpu), torch.empty(C, device=gpu), torch.empty(K, device=gpu)
    dH = torch.empty(M, K, dtype=torch.bfloat16, device=gpu)
    head_backward(dl, go, h, sh[0], dW, db, dH=dH, dbprev=dbp, relu_mask=True)
    for m, b, s, gr in zip(ms, bs, sh, (dW, db, dbp)):
        sgd_flat_(m.view(-1), b.view(-1), gr.view(-1), s.view(-1), lr, mom, wd)
    # fused: the shadow of W is the W operand itself, as in training
    fm, fb, fs = state()
    dH2 = torch.empty_like(dH)
    head_backward(dl, go, h, fs[0], None, None, dH=dH2, relu_mask=True, sgd_w=(fm[0], fb[0], fs[0], lr, mom, wd),
                  sgd_b=(fm[1], fb[1], fs[1], lr, mom, wd), sgd_prev=(fm[2], fb[2], fs[2], lr, mom, wd))
    assert torch.equal(dH, dH2)
    for i, name in enumerate(("W", "bias", "previous bias")):
        assert torch.allclose(fm[i], ms[i], rtol=1e-6, atol=1e-6), name
        if mom:
            assert torch.allclose(fb[i], bs[i], rtol=1e-6, atol=1e-6), name + " momentum"
        assert torch.equal(fs[i], fm[i].to(torch.bfloat16)), name + " shadow"


# ------------------------------------------------------------------ 6. repeatability
def test_repeatable_and_tickets_left_zero(gpu):
    from ddpx.ops.head import head_backward, head_forward
    from ddpx.ops.loss import SoftTargets
    C, K = 100, 512
    h, w, b, a, tb, lam = _real_inputs(gpu, C, 300, K, 3, torch.bfloat16)
    soft = SoftTargets(tb, lam, 0.1)
    first = head_forward(h, w, b, a, soft=soft)
    again = head_forward(h, w, b, a, soft=soft)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    outs = []
    for _ in range(2):
        dW, db, dbp = torch.empty(C, K, device=gpu), torch.empty(C, device=gpu), torch.empty(K, device=gpu)
        dH = torch.empty(300, K, dtype=torch.bfloat16, device=gpu)
        head_backward(first[2], None, h, w, dW, db, dH=dH, dbprev=dbp, relu_mask=True)
        outs.append((dW, db, dbp, dH))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # the tickets are zero again: another batch size (other row blocks, another K split) is still right
    for M in (50, 17):
        loss, logits, _ = head_forward(h[:M], w, b, a[:M])
        z = F.linear(h[:M].double(), w.double(), b.double())
        assert (logits.double() - z).abs().max().item() < 1e-4 * max(1.0, z.abs().max().item())
        ref = F.cross_entropy(logits.double(), a[:M]).item()
        assert abs(loss.item() - ref) < 1e-4 * max(1.0, abs(ref))


def test_limits(gpu):
    from ddpx.ops.head import head_forward
    from ddpx.runtime import native
    h = torch.zeros(4, 32, dtype=torch.bfloat16, device=gpu)
    w = torch.zeros(129, 32, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="128"):
        head_forward(h, w, torch.zeros(129, device=gpu))
    lib = native.kernels()
    nul = [None] * 12
    for C, K, ldh in ((0, 32, 32), (129, 32, 32), (100, 36, 40), (100, 32, 36)):
        assert lib.ddpx_head_fwd(None, None, None, None, 4, K, C, ldh, 1.0, *nul[:7], 0, None, None, None) < 0
    for C, K, ldh in ((0, 32, 32), (129, 32, 32), (100, 24, 24), (100, 32, 36)):
        assert lib.ddpx_head_bwd(None, None, None, None, 4, K, C, ldh, None, 0, 1.0, None, None, None, 0, 0,
                                 *nul[:10], 0.0, 0.0, None) < 0
