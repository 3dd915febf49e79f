"""ResNet-20 (and depth 8, a downsampling block directly on another) on the native bf16 graph with the option-A join
kernels: against the torch fp32 twin of tests/_pad_ref.py with test_gpu_resnet18.py's budget, the fused optimizer
against the unfused path, and a captured Trainer run against the eager one."""
import pytest
import torch
import torch.nn.functional as F

from tests import _pad_ref as R
from tests.test_gpu_resnet import _bf, _rel, _twin

pytestmark = pytest.mark.gpu


def _native(gpu, seed, depth=20):
    import ddpx
    from ddpx.models import ResNetCifar
    torch.manual_seed(seed)
    m = ResNetCifar(depth)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    m.use_native = True
    return m, init, ddpx.prepare_model(m, gpu)


@pytest.mark.parametrize("depth", [8, 20])
def test_resnet20_native_bf16_matches_torch(gpu, depth):
    """test_resnet18_native_bf16_matches_torch's budget, unchanged: loss within 3e-2 * max(1, loss) of fp32, every
    parameter gradient within 3x torch autocast's error + 0.03, running statistics 2e-2, eval logits 5e-2."""
    m, init, _ = _native(gpu, 2, depth)
    ref, amp = _twin(init, gpu), _twin(init, gpu)
    N = 8
    x = _bf(torch.rand(N, 3, 32, 32, device=gpu))
    t = torch.randint(0, 10, (N,), device=gpu)
    loss, logits = m.forward_loss(x, t)
    assert logits is None  # the native path ran
    loss.backward()
    rl = F.cross_entropy(R.twin_forward(ref, x, True, m.n), t)
    rl.backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        al = F.cross_entropy(R.twin_forward(amp, x, True, m.n).float(), t)
    al.backward()
    assert abs(loss.item() - rl.item()) < 3e-2 * max(1.0, rl.item())
    for n, p in m.named_parameters():
        ours, theirs = _rel(p.main_grad, ref[n].grad), _rel(amp[n].grad, ref[n].grad)
        assert ours < 3 * theirs + 0.03, (n, ours, theirs)
    for n, bb in m.named_buffers():
        if bb.dtype == torch.int64:
            assert int(bb) == 1, n
        else:
            assert _rel(bb, ref[n]) < 2e-2, n
    m.eval()
    with torch.no_grad():
        assert _rel(m(x), R.twin_forward(ref, x, False, m.n)) < 5e-2


def test_resnet20_fused_optimizer_equals_unfused(gpu):
    from ddpx.optim.sgd import SGD
    a, b = _native(gpu, 3)[0], _native(gpu, 3)[0]
    oa = SGD(a.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, fused_backward=True)
    ob = SGD(b.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    torch.manual_seed(3)
    for _ in range(2):
        x = torch.rand(8, 3, 32, 32, device=gpu)
        t = torch.randint(0, 10, (8,), device=gpu)
        for m, o in ((a, oa), (b, ob)):
            o.sync_lr()
            o.zero_grad()
            m.forward_loss(x, t)[0].backward()
            o.step()
    for (n, p), q in zip(list(a.named_parameters()) + list(a.named_buffers()), list(b.parameters()) + list(b.buffers())):
        assert torch.equal(p, q), n


def _trainer_run(gpu, graph, steps=4):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    model = _native(gpu, 1)[0]
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
    loader = DeviceLoader(synthetic_cifar(8 * steps, seed=4), 8, gpu, train=True, layout=model.input_layout(gpu),
                          seed=2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
    tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=graph, graph_warmup=2, label_smoothing=0.1)
    tr.train(1)
    torch.cuda.synchronize()
    return tr, opt.flat.master.clone(), opt.momentum_buffer.clone()


def test_resnet20_captured_trainer_equals_eager(gpu, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    eager, w_eager, m_eager = _trainer_run(gpu, False)
    graph, w_graph, m_graph = _trainer_run(gpu, True)
    assert graph._graph is not None, graph.graph_error
    assert eager.global_step == graph.global_step == 4
    assert torch.isfinite(eager.last_loss).item()
    assert torch.equal(eager.last_loss, graph.last_loss)
    assert torch.equal(w_eager, w_graph) and torch.equal(m_eager, m_graph)
