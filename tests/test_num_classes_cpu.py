"""Class counts other than 10 on the CPU: the CIFAR-100 loader, the label check, ``--num_classes`` on the command
line and in the checkpoint, and ``head_forward`` at 100 classes against fp64."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_cifar100(root, n=5, seed=0):
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, 256, size=(n, 3074), dtype=np.uint8)
    rec[:, 0] = rng.integers(0, 20, size=n)            # coarse labels: ignored
    rec[:, 1] = np.array([99, 0, 57, 20, 19])[:n]      # fine labels (some above every coarse label)
    os.makedirs(os.path.join(root, "cifar-100-binary"))
    for split in ("train", "test"):
        rec.tofile(os.path.join(root, "cifar-100-binary", split + ".bin"))
    return rec


def test_load_cifar100_binary(tmp_path):
    from ddpx.data.datasets import get_datasets, load_cifar100
    rec = _write_cifar100(str(tmp_path))
    ds = load_cifar100(str(tmp_path), train=True)
    assert ds.num_classes == 100 and len(ds) == 5
    assert ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (5, 3, 32, 32)
    assert ds.labels.dtype == torch.int64 and ds.labels.tolist() == [99, 0, 57, 20, 19]
    assert np.array_equal(ds.images.numpy().reshape(5, 3072), rec[:, 2:])
    train, test = get_datasets("cifar100", str(tmp_path))
    assert train.num_classes == test.num_classes == 100 and torch.equal(test.labels, ds.labels)
    with pytest.raises(ValueError):
        get_datasets("cifar100", str(tmp_path), num_classes=10)
    with pytest.raises(FileNotFoundError):
        load_cifar100(str(tmp_path / "nowhere"))


def test_label_beyond_num_classes_is_refused():
    from ddpx.data.datasets import check_labels, get_datasets, synthetic_cifar
    ds = synthetic_cifar(32, num_classes=100)
    assert check_labels(ds, 100) is ds
    ds.labels[3] = 100
    with pytest.raises(ValueError, match="100"):
        check_labels(ds, 100)
    train, test = get_datasets("synthetic", train_size=256, test_size=64, num_classes=37)
    assert train.num_classes == test.num_classes == 37 and int(train.labels.max()) < 37
    assert get_datasets("synthetic", train_size=16, test_size=16)[0].num_classes == 10


def test_singlegpu_cpu_100_classes_and_checkpoint(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--device", "cpu", "--model", "mlp",
           "--hidden", "64", "--data", "synthetic", "--num_classes", "100", "--train_size", "512", "--test_size", "256"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "accuracy=" in r.stdout
    sd = torch.load(tmp_path / "checkpoint.pt", map_location="cpu")
    shapes = [tuple(v.shape) for v in sd.values() if torch.is_tensor(v)]
    assert (100, 64) in shapes and (100,) in shapes, shapes


def test_num_classes_against_a_real_dataset_is_an_argument_error(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--device", "cpu", "--data", "cifar10",
           "--num_classes", "100"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
    assert "--num_classes" in r.stderr
    from ddpx.train.app import build_parser, resolve_data_root, resolve_num_classes
    a = build_parser("t").parse_args(["1", "1", "--data", "cifar100"])
    assert resolve_num_classes(a) == 100 and resolve_data_root(a) == "data/cifar100"
    a = build_parser("t").parse_args(["1", "1", "--data", "cifar100", "--data_root", "/x", "--num_classes", "100"])
    assert resolve_num_classes(a) == 100 and resolve_data_root(a) == "/x"
    a = build_parser("t").parse_args(["1", "1", "--data", "synthetic"])
    assert resolve_num_classes(a) == 10 and resolve_data_root(a) == "data/cifar10"


def test_build_model_passes_num_classes():
    from ddpx.models import build_model
    for name, kw in (("vgg", {}), ("deepnn", {}), ("mlp", {"hidden": 64})):
        m = build_model(name, num_classes=100, **kw)
        w, b = list(m.parameters())[-2:]
        assert w.shape[0] == 100 and tuple(b.shape) == (100,), name
        ten = build_model(name, **kw)
        assert list(ten.parameters())[-1].shape == (10,)
        with pytest.raises(RuntimeError):  # another class count does not resume, as in torch
            ten.load_state_dict(m.state_dict())


def test_cpu_head_forward_100_classes_matches_fp64():
    from ddpx.ops.head import head_forward
    from ddpx.ops.loss import SoftTargets
    g = torch.Generator().manual_seed(0)
    M, K, C = 33, 64, 100
    h, w, b = torch.randn(M, K, generator=g), torch.randn(C, K, generator=g) * 0.2, torch.randn(C, generator=g)
    t, tb = torch.randint(0, C, (M,), generator=g), torch.randint(0, C, (M,), generator=g)
    lam = torch.rand(M, generator=g)
    hits = torch.zeros((), dtype=torch.int32)
    loss, logits, dl = head_forward(h, w, b, t, correct=hits)
    z = F.linear(h.double(), w.double(), b.double())
    assert torch.allclose(logits.double(), z, atol=1e-5)
    assert abs(loss.item() - F.cross_entropy(z, t).item()) < 1e-5
    assert torch.allclose(dl.double(), (torch.softmax(z, 1) - F.one_hot(t, C)) / M, atol=1e-7)
    assert hits.item() == (z.argmax(1) == t).sum().item()
    q = lam.double()[:, None] * F.one_hot(t, C) + (1 - lam.double()[:, None]) * F.one_hot(tb, C)
    sl, _, sdl = head_forward(h, w, b, t, soft=SoftTargets(tb, lam, 0.1))
    assert abs(sl.item() - F.cross_entropy(z, q, label_smoothing=0.1).item()) < 1e-5
    assert torch.allclose(sdl.double(), (torch.softmax(z, 1) - (0.9 * q + 0.1 / C)) / M, atol=1e-7)
