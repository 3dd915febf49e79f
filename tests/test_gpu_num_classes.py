"""100 classes through the six native model paths, a captured Trainer run with label smoothing + Mixup + fused SGD,
and the command line: the wide head seen through ``forward_loss`` and the gradient protocol."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = 3
ULP = 2.0 ** -23  # relative spacing of fp32


def _pair(gpu, name, dtype, nc):
    """(native model, torch-op fp32 model) from one init, dropout off, training mode."""
    import ddpx
    from ddpx.models import build_model
    torch.manual_seed(7)
    kw = dict(device=gpu, hidden=512 if name == "mlp" else None, num_classes=nc)
    native = build_model(name, dtype=dtype, kernels="native", **kw)
    ref = build_model(name, dtype="fp32", kernels="torch", **kw)
    ref.load_state_dict(native.state_dict())
    ref.to(gpu)
    for m in (native, ref):
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.train()
    flat = ddpx.prepare_model(native, gpu)
    return native, ref, flat


def _deviation(gpu, name, dtype, nc):
    """Largest deviation over BATCHES batches of (loss, classifier weight gradient, classifier bias gradient)
    between the native path and the torch fp32 engine: |d loss| / |loss|, |d grad|_F / |grad|_F."""
    native, ref, flat = _pair(gpu, name, dtype, nc)
    (wn, wp), (bn, bp) = list(native.named_parameters())[-2:]
    assert tuple(wp.shape)[0] == nc and wp.dim() == 2 and tuple(bp.shape) == (nc,), (wn, bn)
    rp = dict(ref.named_parameters())
    g = torch.Generator().manual_seed(3)
    dev = [0.0, 0.0, 0.0]
    for _ in range(BATCHES):
        x = torch.rand(64, 3, 32, 32, generator=g).to(gpu)
        y = (torch.randint(0, 100, (64,), generator=g) % nc).to(gpu)
        flat.zero_grad()
        loss, logits = native.forward_loss(x, y)
        assert logits is None  # the native path ran
        loss.backward()
        ref.zero_grad()
        rl = F.cross_entropy(ref(x), y)
        rl.backward()
        got = (loss.detach().double(), wp.main_grad.double(), bp.main_grad.double())
        want = (rl.detach().double(), rp[wn].grad.double(), rp[bn].grad.double())
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.isfinite(a).all().item()
            dev[i] = max(dev[i], ((a - b).norm() / b.norm()).item())
    return dev


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["mlp", "vgg", "deepnn"])
def test_native_paths_at_100_classes(gpu, name, dtype):
    """The bar is twice the deviation the 10-class path (code that exists today) shows in the same comparison on
    the same inputs.  Both sides of the comparison are fp32 numbers, the torch engine's included, so no deviation
    resolves below one unit in the last place: the yardstick is floored at 2^-23.  (Without the floor the fp32 MLP's
    loss sits at the quantum: 2.07e-7 = 2 ulp of 4.6 at 100 classes against 1.03e-7 = 1 ulp of 2.3 at 10.)"""
    base = [max(d, ULP) for d in _deviation(gpu, name, dtype, 10)]
    wide = _deviation(gpu, name, dtype, 100)
    for what, d10, d100 in zip(("loss", "classifier weight gradient", "classifier bias gradient"), base, wide):
        print(f"{name} {dtype} {what}: deviation from the torch fp32 engine {d100:.3e} at 100 classes, "
              f"{d10:.3e} at 10 (bar {2 * d10:.3e})")
    for what, d10, d100 in zip(("loss", "weight", "bias"), base, wide):
        assert d100 <= 2 * d10, (what, d100, d10)


def _train(gpu, graph, ckpt_path, steps=6):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.data.mix import MixConfig
    from ddpx.models import MLP
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    torch.manual_seed(1)
    model = MLP(hidden=512, num_classes=100)
    ddpx.prepare_model(model, gpu)
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
    ds = synthetic_cifar(64 * steps, seed=4, num_classes=100)
    loader = DeviceLoader(ds, 64, gpu, train=True, layout="flat_bf16", seed=2, mix=MixConfig(0.2, 1.0))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
    tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=graph, graph_warmup=2, label_smoothing=0.1,
                 ckpt_path=ckpt_path)
    tr.train(1)
    torch.cuda.synchronize()
    return tr, opt.flat.master.clone()


def test_trainer_eager_equals_captured_at_100_classes(gpu, tmp_path):
    eager, w_eager = _train(gpu, False, str(tmp_path / "eager.pt"))
    graph, w_graph = _train(gpu, True, str(tmp_path / "graph.pt"))
    assert graph._graph is not None, graph.graph_error
    assert eager.global_step == graph.global_step == 6
    assert torch.isfinite(eager.last_loss).item() and torch.isfinite(graph.last_loss).item()
    assert torch.equal(eager.last_loss, graph.last_loss)
    assert torch.equal(w_eager, w_graph)


def test_singlegpu_vgg_100_classes(gpu, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--model", "vgg", "--dtype",
                        "bf16", "--data", "synthetic", "--num_classes", "100", "--train_size", "1024", "--test_size",
                        "512"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "accuracy=" in r.stdout, r.stdout[-3000:]
