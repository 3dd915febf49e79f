"""Soft targets on the GPU: ``ddpx_head_fwd_soft`` / ``ddpx_f32_head_fwd_soft`` against fp64 from the kernel's
own logits, the degenerate case bit for bit against the hard entry points, the LR-table advance through the
soft launch, ``forward_loss(soft=)`` on all six native paths, and an eager-versus-captured Trainer run."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 10


def _inputs(gpu, M, K, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(M, K, generator=g)).to(dtype).to(gpu)
    w = (torch.randn(C, K, generator=g) * (2.0 / K ** 0.5)).to(dtype).to(gpu)
    b = (torch.randn(C, generator=g) * 0.1).to(gpu)
    a = torch.randint(0, C, (M,), generator=g).to(gpu)
    tb = torch.randint(0, C, (M,), generator=g).to(gpu)
    lam = torch.rand(M, generator=g)
    lam[0], lam[1], lam[2] = 0.0, 1.0, 0.5
    return h, w, b, a, tb, lam.to(gpu)


def _q64(a, tb, lam, eps):
    q = lam.double()[:, None] * F.one_hot(a, C).double() + (1 - lam.double()[:, None]) * F.one_hot(tb, C).double()
    return q, (1 - eps) * q + eps / C


def _check_head(head_forward, gpu, M, K, eps, dtype, loss_tol):
    from ddpx.ops.loss import SoftTargets
    h, w, b, a, tb, lam = _inputs(gpu, M, K, 11 * M + K, dtype)
    hits = torch.zeros((), dtype=torch.int32, device=gpu)
    kw = {"correct": hits} if dtype == torch.bfloat16 else {}
    loss, logits, dl = head_forward(h, w, b, a, soft=SoftTargets(tb, lam, eps), **kw)
    hard_loss, hard_logits, hard_dl = head_forward(h, w, b, a)
    assert torch.equal(logits, hard_logits)
    z = logits.double()
    q, qs = _q64(a, tb, lam, eps)
    ref = F.cross_entropy(z, q, label_smoothing=eps).item()
    err_loss = abs(loss.item() - ref)
    # dlogits: twice the hard entry point's own error against fp64 on these inputs, plus 8 * 2^-24 / M for
    # forming q in fp32 (three roundings per class, q <= 1)
    p = torch.softmax(z, 1)
    err_hard = (hard_dl.double() - (p - F.one_hot(a, C).double()) / M).abs().max().item()
    err_soft = (dl.double() - (p - qs) / M).abs().max().item()
    bound = 2 * err_hard + 8 * 2.0 ** -24 / M
    print(f"head {dtype} M={M} K={K} eps={eps}: loss err {err_loss:.3e} (tol {loss_tol(ref):.1e}), "
          f"dlogits err soft {err_soft:.3e} hard {err_hard:.3e} bound {bound:.3e}")
    assert err_loss < loss_tol(ref)
    assert err_soft <= bound
    if kw:
        assert hits.item() == (logits.argmax(1) == a).sum().item()
    # degenerate soft targets: the hard launch's bits
    for soft in (SoftTargets(tb, torch.ones_like(lam), 0.0), SoftTargets(None, None, 0.0), SoftTargets(None, lam, 0.0)):
        hits.zero_()
        hits2 = torch.zeros_like(hits)
        got = head_forward(h, w, b, a, soft=soft, **kw)
        want = head_forward(h, w, b, a, **({"correct": hits2} if kw else {}))
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        assert hits.item() == hits2.item()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [16, 17, 48])
def test_head_soft_bf16(gpu, M, K, eps):
    from ddpx.ops.head import head_forward
    _check_head(head_forward, gpu, M, K, eps, torch.bfloat16, lambda ref: 1e-4 * max(1.0, abs(ref)))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [16, 17, 48])
def test_head_soft_fp32(gpu, M, K, eps):
    from ddpx.ops import f32
    _check_head(f32.head_forward, gpu, M, K, eps, torch.float32, lambda ref: 1e-5)


def test_lr_advance_through_the_soft_launch(gpu):
    from ddpx.ops.head import head_forward
    from ddpx.ops.loss import SoftTargets
    h, w, b, a, tb, lam = _inputs(gpu, 48, 256, 5, torch.bfloat16)
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


def _native_model(gpu, name, dtype):
    import ddpx
    from ddpx.models import build_model
    torch.manual_seed(7)
    m = build_model(name, dtype=dtype, device=gpu, hidden=512 if name == "mlp" else None, kernels="native")
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    ddpx.prepare_model(m, gpu)
    m.train()
    return m


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["mlp", "vgg", "deepnn"])
def test_forward_loss_soft_on_native_paths(gpu, name, dtype):
    from ddpx.ops.loss import SoftTargets
    m = _native_model(gpu, name, dtype)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(64, 3, 32, 32, generator=g).to(gpu)
    a = torch.randint(0, C, (64,), generator=g).to(gpu)
    tb = torch.randint(0, C, (64,), generator=g).to(gpu)
    lam, eps = 0.3, 0.1
    lam_t = torch.full((64,), lam, device=gpu)

    def L(t, soft=None):
        loss, logits = m.forward_loss(x, t, soft=soft) if soft is not None else m.forward_loss(x, t)
        assert logits is None  # the native path ran
        return loss.detach()

    La = L(a)
    for soft in (SoftTargets(), SoftTargets(tb, torch.ones_like(lam_t), 0.0), SoftTargets(None, None, 0.0)):
        assert torch.equal(L(a, soft), La)
    Lb, Lu = L(tb), L(a, SoftTargets(label_smoothing=1.0))
    got = L(a, SoftTargets(tb, lam_t, eps)).item()
    want = (1 - eps) * (lam * La.item() + (1 - lam) * Lb.item()) + eps * Lu.item()
    print(f"{name} {dtype}: L = {got:.7f}, from four hard / uniform losses {want:.7f}, diff {abs(got - want):.2e}")
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    # and the gradient follows: backward through the soft loss runs the untouched backward kernels
    loss, _ = m.forward_loss(x, a, soft=SoftTargets(tb, lam_t, eps))
    loss.backward()
    torch.cuda.synchronize()


def _train(gpu, graph, ckpt_path, steps=6):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.data.mix import MixConfig
    from ddpx.models import MLP
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    torch.manual_seed(1)
    model = MLP(hidden=512)
    ddpx.prepare_model(model, gpu)
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
    ds = synthetic_cifar(64 * steps, seed=4)
    loader = DeviceLoader(ds, 64, gpu, train=True, layout="flat_bf16", seed=2, mix=MixConfig(0.2, 1.0))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
    tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=graph, graph_warmup=2, label_smoothing=0.1,
                 ckpt_path=ckpt_path)
    tr.train(1)  # (with the device LR table: the soft head launch advances it inside the captured step)
    torch.cuda.synchronize()
    return tr, opt.flat.master.clone()


def test_trainer_eager_equals_captured(gpu, tmp_path):
    eager, w_eager = _train(gpu, False, str(tmp_path / "eager.pt"))
    graph, w_graph = _train(gpu, True, str(tmp_path / "graph.pt"))
    assert graph._graph is not None, graph.graph_error
    assert eager.global_step == graph.global_step == 6
    assert torch.isfinite(eager.last_loss).item() and torch.isfinite(graph.last_loss).item()
    assert torch.equal(eager.last_loss, graph.last_loss)
    assert torch.equal(w_eager, w_graph)
