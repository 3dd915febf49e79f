"""The pre-activation ResNet-18/34 on the native bf16 graph (ops/vgg_native.py with ``preact_add`` and
``bn_backward(gadd=)``): against torch with tests/test_gpu_resnet18.py's budgets, a captured Trainer run against the
eager one, and one command-line run.  The torch reference is the functional twin of tests/_preact_ref.py."""
import os

import pytest
import torch

from tests import _preact_ref as P
from tests import test_gpu_resnet18 as R18
from tests.test_gpu_entrypoints import ROOT, _run

pytestmark = pytest.mark.gpu


def _native(gpu, seed):
    import ddpx
    from ddpx.models import PreActResNet
    torch.manual_seed(seed)
    m = PreActResNet(18)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    m.use_native = True
    return m, init, ddpx.prepare_model(m, gpu)


@pytest.fixture
def r18(monkeypatch):
    """tests/test_gpu_resnet18.py with its model factory and its functional twin replaced by this network's: its
    test bodies then hold this model to their budgets, unchanged."""
    monkeypatch.setattr(R18, "_native", _native)
    monkeypatch.setattr(R18, "J", P)
    return R18


def test_preact18_native_bf16_matches_torch(gpu, r18):
    """Loss within 3e-2 * max(1, loss) of the fp32 twin, every parameter gradient within 3x torch autocast's error +
    0.03, running statistics 2e-2, eval logits 5e-2 (the evaluation forward runs the one-pass add + apply)."""
    r18.test_resnet18_native_bf16_matches_torch(gpu)


def test_preact18_captured_trainer_equals_eager(gpu, r18, tmp_path, monkeypatch):
    """Four Trainer steps with the fused SGD, two eager warm-up steps and two replays of the captured step, against
    four eager ones: the same loss, weights and momentum, bit for bit."""
    r18.test_resnet18_captured_trainer_equals_eager(gpu, tmp_path, monkeypatch)


def test_preact34_singlegpu_graph(gpu, tmp_path):
    out = _run([os.path.join(ROOT, "singlegpu.py"), "1", "1", "--model", "preact_resnet34", "--data", "synthetic",
                "--train_size", "2560", "--test_size", "512", "--dtype", "bf16", "--graph"], tmp_path)
    assert "[GPU0] Epoch 0 | Batchsize: 512 | Steps: 5" in out and "note: --graph ignored" not in out
