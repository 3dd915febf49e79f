"""Soft targets on the CPU: ``head_forward(..., soft=)`` against fp64 ``F.cross_entropy`` with probability
targets, the degenerate case against the hard path, the models' ``forward_loss(soft=)`` and the Trainer."""
import pytest
import torch
import torch.nn.functional as F

from ddpx.ops.head import head_forward
from ddpx.ops.loss import SoftTargets


def _case(M=17, K=64, C=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, K, generator=g)
    w = torch.randn(C, K, generator=g) * 0.2
    b = torch.randn(C, generator=g) * 0.1
    a = torch.randint(0, C, (M,), generator=g)
    tb = torch.randint(0, C, (M,), generator=g)
    lam = torch.rand(M, generator=g)
    lam[0], lam[1] = 0.0, 1.0
    return h, w, b, a, tb, lam


def _q64(a, tb, lam, C):
    q = F.one_hot(a, C).double()
    if tb is not None:
        l = lam.double()[:, None] if lam is not None else torch.ones(a.numel(), 1, dtype=torch.float64)
        q = l * q + (1 - l) * F.one_hot(tb, C).double()
    return q


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_cpu_head_forward_soft_matches_fp64(eps, mixed):
    h, w, b, a, tb, lam = _case()
    soft = SoftTargets(tb if mixed else None, lam if mixed else None, eps)
    loss, logits, dl = head_forward(h, w, b, a, soft=soft)
    z = logits.double().requires_grad_(True)
    q = _q64(a, tb if mixed else None, lam if mixed else None, 10)
    ref = F.cross_entropy(z, q, label_smoothing=eps)
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) < 1e-6 * max(1.0, abs(float(ref.detach())))
    assert torch.allclose(dl.double(), z.grad, atol=1e-7, rtol=0)
    if not mixed:  # smoothing alone is F.cross_entropy's own label_smoothing with class targets
        assert abs(float(loss) - float(F.cross_entropy(logits.double(), a, label_smoothing=eps))) < 1e-6
    # the hit count stays against the first labels
    hits = torch.zeros((), dtype=torch.int32)
    head_forward(h, w, b, a, soft=soft, correct=hits)
    assert int(hits) == int((logits.argmax(1) == a).sum())


def test_degenerate_soft_is_the_hard_path():
    h, w, b, a, tb, lam = _case()
    hard = head_forward(h, w, b, a)
    for soft in (SoftTargets(), SoftTargets(tb, torch.ones_like(lam), 0.0), SoftTargets(tb, None, 0.0)):
        got = head_forward(h, w, b, a, soft=soft)
        for x, y in zip(got, hard):
            assert torch.equal(x, y)
    # longer (persistent) buffers: the first M elements count
    big = SoftTargets(torch.cat([tb, tb]), torch.cat([lam, lam]), 0.1)
    assert torch.equal(head_forward(h, w, b, a, soft=big)[0], head_forward(h, w, b, a, soft=SoftTargets(tb, lam, 0.1))[0])


def test_soft_targets_validation():
    with pytest.raises(ValueError):
        SoftTargets(label_smoothing=1.5)
    with pytest.raises(ValueError):
        SoftTargets(tgt_b=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        SoftTargets(lam=torch.zeros(4, dtype=torch.float64))
    h, w, b, a, tb, lam = _case()
    with pytest.raises(ValueError):
        head_forward(h, w, b, a, soft=SoftTargets(tb[:5], lam[:5]))


@pytest.mark.parametrize("name", ["mlp", "vgg", "deepnn"])
def test_forward_loss_soft_on_cpu_models(name):
    from ddpx.models import MLP, VGG, DeepNN
    torch.manual_seed(0)
    model = {"mlp": lambda: MLP(hidden=64), "vgg": VGG, "deepnn": DeepNN}[name]()
    model.eval()  # (dropout / batch statistics off: the calls below see the same network)
    x = torch.rand(6, 3, 32, 32)
    a = torch.randint(0, 10, (6,))
    tb = torch.randint(0, 10, (6,))
    lam = torch.full((6,), 0.3)
    with torch.no_grad():
        hard, _ = model.forward_loss(x, a)
        assert torch.equal(model.forward_loss(x, a, soft=None)[0], hard)
        other, _ = model.forward_loss(x, tb)
        uni, _ = model.forward_loss(x, a, soft=SoftTargets(label_smoothing=1.0))
        got, _ = model.forward_loss(x, a, soft=SoftTargets(tb, lam, 0.1))
    want = 0.9 * (0.3 * float(hard) + 0.7 * float(other)) + 0.1 * float(uni)
    assert abs(float(got) - want) < 1e-5 * max(1.0, abs(want))


def test_trainer_label_smoothing_and_mixing_cpu():
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.data.mix import MixConfig
    from ddpx.models import MLP
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer

    def run(**kw):
        torch.manual_seed(0)
        model = MLP(hidden=64)
        ddpx.prepare_model(model, torch.device("cpu"))
        opt = SGD(model.parameters(), lr=0.05, momentum=0.9)
        ds = synthetic_cifar(128, seed=2)
        loader = DeviceLoader(ds, 64, "cpu", train=True, layout="flat_f32", seed=1, mix=kw.pop("mix", None))
        tr = Trainer(model, loader, opt, 0, 10 ** 9, torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0), **kw)
        tr._run_epoch(0)
        return tr, [p.detach().clone() for p in model.parameters()]

    plain, w0 = run()
    assert plain.soft is None
    again, w1 = run(label_smoothing=0.0)
    assert again.soft is None and all(torch.equal(a, b) for a, b in zip(w0, w1))
    soft, w2 = run(label_smoothing=0.1, mix=MixConfig(0.2, 1.0))
    assert soft.soft.label_smoothing == 0.1 and soft.soft.tgt_b is soft.train_data.soft_targets.tgt_b
    assert torch.isfinite(soft.last_loss) and any(not torch.equal(a, b) for a, b in zip(w0, w2))
    _, w3 = run(label_smoothing=0.1, mix=MixConfig(0.2, 1.0))
    assert all(torch.equal(a, b) for a, b in zip(w2, w3))
