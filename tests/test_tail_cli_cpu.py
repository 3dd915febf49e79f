"""``--resnet_tail`` / ``--tail_scale`` / ``--cutout`` / ``--tta_flip``: parser defaults and argument errors, the
checkpoint record of the tail, and a CPU ``singlegpu.py`` run with all four."""
import os
import re

import pytest
import torch

from tests.test_entrypoints import ROOT, _run


def _parse(*flags):
    from ddpx.train.app import build_parser
    return build_parser("t").parse_args(["1", "1", *flags])


def test_parser_defaults():
    a = _parse()
    assert (a.resnet_tail, a.tail_scale, a.cutout, a.tta_flip) == ("avg", 1.0, 0, False)
    a = _parse("--model", "resnet9", "--resnet_tail", "max", "--tail_scale", "0.125", "--cutout", "8", "--tta_flip")
    assert (a.resnet_tail, a.tail_scale, a.cutout, a.tta_flip) == ("max", 0.125, 8, True)
    assert _parse("--model", "resnet9", "--resnet_tail", "max").tail_scale == 1.0
    assert _parse("--model", "vgg", "--cutout", "8", "--tta_flip").cutout == 8  # Cutout and TTA serve every model


@pytest.mark.parametrize("flags,message", [
    (["--resnet_tail", "max"], "apply to --model resnet9 only"),                 # the default model is vgg
    (["--model", "mlp", "--tail_scale", "0.125"], "apply to --model resnet9 only"),
    (["--model", "deepnn", "--resnet_tail", "max", "--tail_scale", "0.125"], "apply to --model resnet9 only"),
    (["--model", "resnet9", "--tail_scale", "0.125"], "--tail_scale needs --resnet_tail max"),
    (["--model", "resnet9", "--resnet_tail", "median"], "argument --resnet_tail: invalid choice: 'median'"),
    (["--model", "resnet9", "--cutout", "-1"], "--cutout must not be negative"),
])
def test_argument_errors(flags, message, capsys):
    """Each case's own validation fires: the error text, not just an exit (an unknown flag exits too)."""
    with pytest.raises(SystemExit):
        _parse(*flags)
    assert message in capsys.readouterr().err


def test_build_model_and_optimizer_builds_the_tail():
    from ddpx.train.app import build_model_and_optimizer
    args = _parse("--model", "resnet9", "--resnet_tail", "max", "--tail_scale", "0.125", "--device", "cpu")
    model, _ = build_model_and_optimizer(args, torch.device("cpu"))
    assert (model.tail, model.tail_scale) == ("max", 0.125)
    model, _ = build_model_and_optimizer(_parse("--model", "resnet9", "--device", "cpu"), torch.device("cpu"))
    assert (model.tail, model.tail_scale) == ("avg", 1.0)


def test_full_checkpoint_records_the_tail_and_refuses_another(tmp_path):
    from ddpx.models import ResNet9
    from ddpx.train import checkpoint as ckpt
    torch.manual_seed(0)
    m = ResNet9(tail="max", tail_scale=0.125)
    assert ckpt.tail_record(m) == {"tail": "max", "tail_scale": 0.125}
    assert ckpt.tail_record(ResNet9()) == {} and ckpt.tail_record(torch.nn.Linear(2, 2)) == {}
    path = str(tmp_path / "full.pt")
    ckpt.save_full_checkpoint(path, m, None, None, 3, extra=ckpt.tail_record(m))
    state = torch.load(path, weights_only=True)
    assert state["extra"] == {"tail": "max", "tail_scale": 0.125}
    assert tuple(state["model"].keys()) == ResNet9.STATE_KEYS
    again = ResNet9(tail="max", tail_scale=0.125)
    assert ckpt.load_full_checkpoint(path, again) == 4
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), again.state_dict().values()))
    for other in (ResNet9(), ResNet9(tail="max"), ResNet9(tail="max", tail_scale=0.25)):
        with pytest.raises(ValueError, match=r"tail='max' tail_scale=0\.125.*tail=") as e:
            ckpt.load_full_checkpoint(path, other)
        assert f"tail={other.tail!r} tail_scale={other.tail_scale:g}" in str(e.value)  # both are named
    # a file of the default tail holds no record and loads into the default model only
    plain = str(tmp_path / "plain.pt")
    ckpt.save_full_checkpoint(plain, ResNet9(), None, None, 0, extra=ckpt.tail_record(ResNet9()))
    assert torch.load(plain, weights_only=True)["extra"] == {}
    assert ckpt.load_full_checkpoint(plain, ResNet9()) == 1
    with pytest.raises(ValueError):
        ckpt.load_full_checkpoint(plain, m)


def test_singlegpu_script_runs_the_published_recipe_on_cpu(tmp_path):
    from ddpx.models import ResNet9
    cmd = [os.path.join(ROOT, "singlegpu.py"), "1", "1", "--model", "resnet9", "--resnet_tail", "max", "--tail_scale",
           "0.125", "--cutout", "8", "--tta_flip", "--data", "synthetic", "--batch_size", "16", "--device", "cpu",
           "--train_size", "32", "--test_size", "16", "--ema_decay", "0.9", "--eval_every", "1", "--full_checkpoint"]
    out = _run(cmd, tmp_path)
    lines = out.splitlines()
    assert "Epoch 0 | Training checkpoint saved at checkpoint.pt" in lines
    assert any(re.fullmatch(r"fp32 model has accuracy=\d+\.\d\d%", ln) for ln in lines), out[-2000:]
    assert any(re.fullmatch(r"EMA model has accuracy=\d+\.\d\d%", ln) for ln in lines), out[-2000:]
    sd = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    assert tuple(sd.keys()) == ResNet9.STATE_KEYS
    full = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)
    assert full["extra"]["tail"] == "max" and full["extra"]["tail_scale"] == 0.125
