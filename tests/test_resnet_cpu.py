"""ResNet-9 on the CPU: structure, the independent functional twin, the script run, and the float64 references of
the residual BatchNorm kernels (tests/_resnet_ref.py) against CPU autograd."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X
from tests import _resnet_ref as R
from tests.test_entrypoints import ROOT, _run


def _model(num_classes=10, seed=0):
    from ddpx.models import build_model
    torch.manual_seed(seed)
    return build_model("resnet9", device="cpu", num_classes=num_classes)


def test_structure():
    from ddpx.models import ResNet9
    m = _model()
    assert isinstance(m, ResNet9)
    assert sum(p.numel() for p in m.parameters()) == 6_573_130
    assert sum(p.numel() for p in _model(100).parameters()) == 6_573_130 + 90 * 513
    assert tuple(m.state_dict().keys()) == ResNet9.STATE_KEYS
    assert len(ResNet9.STATE_KEYS) == 8 * 6 + 2
    assert [k for k in ResNet9.STATE_KEYS if "res1.1" in k] == [
        "res1.1.conv.weight", "res1.1.bn.weight", "res1.1.bn.bias", "res1.1.bn.running_mean",
        "res1.1.bn.running_var", "res1.1.bn.num_batches_tracked"]
    assert all(c.bias is None and c.kernel_size == (3, 3) and c.padding == (1, 1) and c.stride == (1, 1)
               for c in m.modules() if isinstance(c, torch.nn.Conv2d))
    # registration order == forward order: the order in which forward hooks fire on the leaf modules
    leaves = [mod for mod in m.modules() if not list(mod.children())]
    fired = []
    hooks = [mod.register_forward_hook(lambda mod, i, o: fired.append(mod)) for mod in leaves]
    m(torch.randn(2, 3, 32, 32))
    for h in hooks:
        h.remove()
    assert len(fired) == len(leaves) and all(a is b for a, b in zip(fired, leaves))
    # the native graphs' description agrees with the modules
    nb = m.native_blocks()
    assert [(c.in_channels, c.out_channels, pool, skip) for c, _, pool, skip in nb] == [
        (3, 64, False, None), (64, 128, True, None), (128, 128, False, None), (128, 128, False, 1),
        (128, 256, True, None), (256, 512, True, None), (512, 512, False, None), (512, 512, False, 5)]
    assert [p for c, bn, _, _ in nb for p in (c.weight, bn.weight, bn.bias)] == list(m.parameters())[:-2]


@pytest.mark.parametrize("training", [True, False])
def test_model_equals_independent_twin(training):
    m = _model(seed=3)
    for mod in m.modules():  # non-trivial BatchNorm parameters and running statistics
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.5, 2.0)
    m.train(training)
    sd = R.twin_state(m)
    x = torch.randn(6, 3, 32, 32)
    t = torch.randint(0, 10, (6,))
    out = m(x)
    ref = R.twin_forward(sd, x, training)
    assert out.shape == (6, 10)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5), float((out - ref).abs().max())
    F.cross_entropy(out, t).backward()
    F.cross_entropy(ref, t).backward()
    for k, p in m.named_parameters():
        scale = float(p.grad.abs().max()) + 1e-12
        err = float((p.grad - sd[k].grad).abs().max())
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)
    for k, v in m.state_dict().items():  # the running statistics moved alike
        if "running" in k or "num_batches" in k:
            if "num_batches" in k:
                continue  # F.batch_norm does not count batches; the modules do
            assert torch.allclose(v, sd[k], rtol=1e-5, atol=1e-6), k
    if training:
        assert all(int(v) == 1 for k, v in m.state_dict().items() if "num_batches" in k)
    # forward_loss on the CPU is the torch-op path
    loss, logits = m.forward_loss(x, t)
    assert logits is not None and torch.isfinite(loss)


def test_twin_has_a_real_skip():
    """The twin (and so the model) is not a plain chain: zeroing the branch leaves the skip path."""
    m = _model(seed=1).eval()
    sd = R.twin_state(m)
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        base = R.twin_forward(sd, x, False)
        for k in ("res1.1.bn.weight", "res1.1.bn.bias", "res3.1.bn.weight", "res3.1.bn.bias"):
            sd[k].zero_()
        cut = R.twin_forward(sd, x, False)
        m.res1[1].bn.weight.zero_(), m.res1[1].bn.bias.zero_(), m.res3[1].bn.weight.zero_(), m.res3[1].bn.bias.zero_()
        assert torch.allclose(m(x), cut, rtol=1e-5, atol=1e-5)
    assert cut.abs().max() > 0 and not torch.allclose(base, cut)


def test_singlegpu_script_trains_resnet9_on_cpu(tmp_path):
    from ddpx.models import ResNet9
    out = _run([os.path.join(ROOT, "singlegpu.py"), "1", "1", "--model", "resnet9", "--batch_size", "16", "--device",
                "cpu", "--data", "synthetic", "--train_size", "32", "--test_size", "16"], tmp_path)
    assert "Epoch 0 | Training checkpoint saved at checkpoint.pt" in out.splitlines()
    sd = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    assert tuple(sd.keys()) == ResNet9.STATE_KEYS
    ResNet9().load_state_dict(sd, strict=True)


def test_num_classes_100_builds_wide_classifier():
    from ddpx.train.app import build_model_and_optimizer, build_parser
    args = build_parser("resnet9").parse_args(["1", "1", "--model", "resnet9", "--num_classes", "100", "--device",
                                                "cpu"])
    model, _ = build_model_and_optimizer(args, torch.device("cpu"))
    assert tuple(model.classifier.weight.shape) == (100, 512)
    assert model(torch.randn(2, 3, 32, 32)).shape == (2, 100)


# ------------------------------------------------------------------ the float64 references against autograd
@pytest.mark.parametrize("shape", X.BN_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_apply_res_ref_matches_torch(shape):
    c = R.res_case(shape, False)
    got = R.apply_res_ref(c["y"], c["a"], c["b"], c["res"])
    want = c["res"] + F.relu(c["y"] * c["a"] + c["b"])
    assert torch.equal(got, want)
    assert got.abs().max() <= 26 and torch.equal(got * 4, (got * 4).round())
    assert torch.equal(got.to(torch.bfloat16).double(), got)  # exactly representable in bf16


@pytest.mark.parametrize("pool", [False, True])
def test_two_gradient_refs_match_autograd(pool):
    """The block below a residual block: out feeds the branch and the skip, so autograd delivers g1 + g2."""
    shape = X.BN_SHAPES[1]
    c = R.res_case(shape, pool)
    y, a, b, g1, g2 = (c[k] for k in ("y", "a", "b", "g", "g2"))
    b = b + 0.1  # keeps z = a*y + b away from 0 (as tests/test_exact_refs_cpu.py)
    mu = y.mean((0, 1, 2))
    rs = 1.0 / (y.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()
    gamma, beta = a / rs, b + mu * a
    yr, gr, br = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    xh = (yr - yr.mean((0, 1, 2))) / (yr.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()
    out = F.relu(xh * gr + br).permute(0, 3, 1, 2)
    if pool:
        out = F.max_pool2d(out, 2)
    branch, skip = out * 1.0, out * 1.0  # two consumers of the block's output
    torch.autograd.backward([branch, skip], [g1.permute(0, 3, 1, 2).contiguous(), g2.permute(0, 3, 1, 2).contiguous()])
    dy, dgamma, dbeta, terms = R.bn_backward_ref_2g(g1, g2, y, a, b, mu, rs, pool)
    assert torch.allclose(dy, yr.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(dgamma, gr.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(dbeta, br.grad, rtol=1e-9, atol=1e-9)
    assert torch.equal(R.route_ref_2g(g1, g2, y, a, b, pool), X.route_ref(g1 + g2, y, a, b, pool))
    assert torch.equal(dbeta, R.route_ref_2g(g1, g2, y, a, b, pool).sum((0, 1, 2)))
    assert terms.shape == y.shape


def test_unrounded_case_separates_a_rounded_sum():
    """On the {-64, 64} + {-0.25, 0.25} case a bf16 round of g1 + g2 changes dbeta and dgamma, and the exactness
    conditions hold on every BN shape used."""
    for shape in X.BN_SHAPES:
        for pool in (False, True):
            c = R.unrounded_case(shape, pool)
            s = c["g"] + c["g2"]
            assert not torch.equal(s.to(torch.bfloat16).double(), s)
            xhat = (c["y"] - c["mean"]) * c["rstd"]
            gz = R.route_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], pool)
            R.require_exact_sums(gz, xhat, g_unit=4, x_unit=8)
            _, dg, db, _ = R.bn_backward_ref_2g(c["g"], c["g2"], c["y"], c["a"], c["b"], c["mean"], c["rstd"], pool)
            _, dgr, dbr, _ = X.bn_backward_ref(s.to(torch.bfloat16).double(), c["y"], c["a"], c["b"], c["mean"],
                                               c["rstd"], pool)
            assert not torch.equal(db, dbr) and not torch.equal(dg, dgr)
            c2 = R.res_case(shape, pool)
            R.require_exact_sums(R.route_ref_2g(c2["g"], c2["g2"], c2["y"], c2["a"], c2["b"], pool),
                                 (c2["y"] - c2["mean"]) * c2["rstd"])
