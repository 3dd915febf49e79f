"""Validation during training on the GPU must not disturb training: the toy MLP's weights and momentum with a
validation after every epoch are bitwise those without, eager and under a captured step (whose graph stays the one
captured before the first evaluation); an evaluation between VGG steps leaves weights and BatchNorm running
statistics bitwise alone; and ``evaluate_metrics``' top-1 is ``evaluate()``'s float."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mlp_run(gpu, tmp_path, graph, validate):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.models import MLP
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    torch.manual_seed(1)
    model = MLP(hidden=256)
    ddpx.prepare_model(model, gpu)
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
    loader = DeviceLoader(synthetic_cifar(64 * 4, seed=4), 64, gpu, train=True, layout="flat_bf16", seed=2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
    kw = {}
    if validate:
        kw = dict(val_data=DeviceLoader(synthetic_cifar(150, seed=5), 64, gpu, train=False, layout="flat_bf16"),
                  eval_every=1, topk=5)
    tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=graph, graph_warmup=2,
                 ckpt_path=str(tmp_path / f"ckpt_{graph}_{validate}.pt"), **kw)
    seen = []
    if validate:
        inner = tr._validate

        def spy(epoch):
            before = tr._graph
            res = inner(epoch)
            seen.append((before, tr._graph, res))
            return res
        tr._validate = spy
    tr.train(2)
    torch.cuda.synchronize()
    return tr, opt.flat.master.clone(), opt.flat.state_tensors["momentum"].clone(), seen


@pytest.mark.parametrize("graph", [False, True])
def test_mlp_training_is_bitwise_the_same_with_validation(gpu, tmp_path, graph):
    plain, w0, m0, _ = _mlp_run(gpu, tmp_path, graph, validate=False)
    tr, w1, m1, seen = _mlp_run(gpu, tmp_path, graph, validate=True)
    assert torch.equal(w0, w1) and torch.equal(m0, m1)
    assert m0.abs().sum().item() > 0
    assert len(seen) == 2 and all(r.samples == 150 and r.k == 5 and r.loss == r.loss for _, _, r in seen)
    if graph:
        assert plain.graph_error is None and tr.graph_error is None
        first = seen[0][0]
        assert first is not None, "the step was captured in epoch 0, before the first evaluation"
        assert all(b is first and a is first for b, a, _ in seen) and tr._graph is first
    else:
        assert tr._graph is None


def test_vgg_evaluation_between_steps_changes_nothing(gpu):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.models import build_model
    from ddpx.optim import SGD
    from ddpx.train.evaluate import evaluate, evaluate_metrics
    torch.manual_seed(7)
    m = build_model("vgg", dtype="bf16", device=gpu, kernels="native")
    ddpx.prepare_model(m, gpu)
    m.train()
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    layout = m.input_layout(gpu)
    train = DeviceLoader(synthetic_cifar(32 * 3, seed=4), 32, gpu, train=True, layout=layout, seed=2)
    val = DeviceLoader(synthetic_cifar(70, seed=5), 32, gpu, train=False, layout=layout)

    def steps():
        for x, y in train:
            opt.zero_grad()
            loss, _ = m.forward_loss(x, y)
            loss.backward()
            opt.step()

    def state():
        torch.cuda.synchronize()
        bufs = {k: v.detach().clone() for k, v in m.named_buffers()}
        return opt.flat.master.clone(), opt.flat.state_tensors["momentum"].clone(), bufs

    steps()
    w0, mom0, b0 = state()
    assert any("running_mean" in k for k in b0)
    res = evaluate_metrics(m, val, topk=5, progress=False)
    w1, mom1, b1 = state()
    assert m.training
    assert torch.equal(w0, w1) and torch.equal(mom0, mom1)
    assert b0.keys() == b1.keys() and all(torch.equal(b0[k], b1[k]) for k in b0)
    old = evaluate(m, val, progress=False)
    assert res.top1 == old and res.samples == 70 and res.top1 <= res.topk <= 100.0 and res.loss == res.loss
    steps()  # and training goes on
    w2, _, b2 = state()
    assert not torch.equal(w2, w1) and any(not torch.equal(b2[k], b1[k]) for k in b1)
