"""``ddpx.optim.WeightEMA`` on the CPU: the weight schedule against its closed form, the buffer against a replay of
``Tensor.lerp_`` bit for bit, serialisation, ``applied()``, and ``singlegpu.py --ema_decay`` end to end."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import ddpx
from ddpx.models import MLP
from ddpx.ops.ema import ema_flat_, ema_weight
from ddpx.optim import SGD, AdamW, WeightEMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _model(kind, seed=0, **ema_kw):
    torch.manual_seed(seed)
    m = MLP(hidden=64)
    ddpx.prepare_model(m, CPU)
    if kind == "sgd":
        o = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    else:
        o = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    return m, o, WeightEMA(o, **ema_kw)


def _step(m, o, s):
    g = torch.Generator().manual_seed(100 + s)
    x = torch.rand(16, 3072, generator=g)
    y = torch.randint(0, 10, (16,), generator=g)
    o.zero_grad()
    loss, _ = m.forward_loss(x, y)
    loss.backward()
    o.step()


@pytest.mark.parametrize("warmup", [False, True])
def test_weight_every_1_is_the_closed_form(warmup):
    decay, u = 0.999, 0
    for s in range(1, 41):
        u, w = ema_weight(s, u, decay, warmup, 1)
        assert u == s
        d = min(decay, (1.0 + s) / (10.0 + s)) if warmup else decay
        assert w == _f32(1.0 - d), (s, w)
    assert ema_weight(40, 39, 0.999, True, 1)[1] == _f32(1.0 - 41.0 / 50.0)  # warm-up still below the decay
    assert ema_weight(9000, 8999, 0.999, True, 1)[1] == _f32(1.0 - 0.999)    # and past it


def test_weight_every_3_skips_two_steps_of_three():
    decay, u = 0.99, 0
    for s in range(1, 41):
        u0 = u
        u, w = ema_weight(s, u, decay, False, 3)
        if s % 3:
            assert w == 0.0 and u == u0, s
        else:
            assert u == u0 + 1 == s // 3 and w == _f32(1.0 - decay ** 3.0), (s, w)
    u, w = ema_weight(6, 1, decay, True, 3)  # warm-up: the update count, not the step, sets the decay
    assert u == 2 and w == _f32(1.0 - (3.0 / 12.0) ** 3.0)
    with pytest.raises(ValueError):
        ema_weight(1, 0, 1.0, False, 1)
    with pytest.raises(ValueError):
        ema_weight(1, 0, 0.9, False, 0)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("kw", [dict(decay=0.999), dict(decay=0.99, warmup=True), dict(decay=0.99, every=2)],
                         ids=["plain", "warmup", "every2"])
def test_buffer_is_bitwise_a_lerp_replay(kind, kw):
    m, o, ema = _model(kind, **kw)
    assert o.ema is ema and ema.buffer is o.flat.state_tensors["ema"]
    assert torch.equal(ema.buffer, o.flat.master)
    replay = [p.detach().clone() for p in m.parameters()]
    u = 0
    for s in range(1, 6):
        before = ema.buffer.clone()
        _step(m, o, s)
        u, w = ema_weight(s, u, kw["decay"], kw.get("warmup", False), kw.get("every", 1))
        if w == 0.0:
            assert torch.equal(ema.buffer, before), s  # a step without update leaves every bit
        else:
            for r, p in zip(replay, m.parameters()):
                r.lerp_(p.detach(), w)
        assert ema.counts() == (s, u)
        for r, p in zip(replay, m.parameters()):
            i = o.flat.index[id(p)]
            assert torch.equal(ema.buffer[o.flat.slice(i)].view(p.shape), r), (s, i)
    assert not torch.equal(ema.buffer, o.flat.master)


def test_zero_weight_touches_nothing_and_lerp_is_the_fma_form():
    e = torch.randn(1000)
    p = torch.randn(1000)
    p[::7] = float("nan")
    p[3::7] = float("inf")
    keep = e.clone()
    ema_flat_(e, p, 0.0)
    assert torch.equal(e, keep)
    # while w < 0.5 torch's lerp_ is e + (p - e) * w with one fused multiply-add: the GPU kernel's two roundings
    e, p = torch.randn(1 << 16), torch.randn(1 << 16)
    w = _f32(1.0 - 0.999)
    d = (p - e).double()  # p - e rounded to fp32, then an exact product and ONE rounding of the sum
    assert torch.equal(e.clone().lerp_(p, w), (e.double() + d * w).float())


def test_state_dict_round_trip_then_the_same_next_step():
    m, o, ema = _model("adamw", decay=0.99, warmup=True)
    for s in range(1, 4):
        _step(m, o, s)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "every", "steps", "updates", "params"}
    assert (sd["decay"], sd["warmup"], sd["every"], sd["steps"], sd["updates"]) == (0.99, True, 1, 3, 3)
    assert set(sd["params"]) == {k for k, _ in m.named_parameters()}
    # the params entry alone loads into a model
    fresh = MLP(hidden=64)
    res = fresh.load_state_dict(sd["params"], strict=False)
    assert not res.unexpected_keys
    assert all(torch.equal(p, sd["params"][k]) for k, p in fresh.named_parameters())
    # a fresh pair with the same weights and optimizer state, the average loaded: the next step gives the same bits
    m2, o2, ema2 = _model("adamw", seed=1, decay=0.99, warmup=True)
    m2.load_state_dict(m.state_dict())
    o2.load_state_dict(o.state_dict())
    ema2.load_state_dict(sd)
    assert ema2.counts() == (3, 3) and torch.equal(ema2.buffer, ema.buffer)
    _step(m, o, 4)
    _step(m2, o2, 4)
    assert torch.equal(o2.flat.master, o.flat.master)
    assert torch.equal(ema2.buffer, ema.buffer) and ema2.counts() == (4, 4)
    bad = dict(sd, params={k: v for k, v in list(sd["params"].items())[1:]})
    with pytest.raises(ValueError, match="no average"):
        ema2.load_state_dict(bad)


def test_applied_swaps_in_and_out_without_changing_a_bit():
    m, o, ema = _model("sgd", decay=0.9)
    for s in range(1, 4):
        _step(m, o, s)
    f = o.flat
    master, buf = f.master.clone(), ema.buffer.clone()
    shadow = f.shadow.clone() if f.shadow is not None else None
    want = ema.state_dict()["params"]
    with ema.applied() as inside:
        assert inside is ema
        sd = m.state_dict()
        assert all(torch.equal(sd[k], v) for k, v in want.items())
        assert torch.equal(ema.buffer, master)  # the training weights wait in the buffer
    with ema.applied():
        pass
    assert torch.equal(f.master, master) and torch.equal(ema.buffer, buf)
    if shadow is not None:
        assert torch.equal(f.shadow, shadow)


def test_applied_refreshes_the_bf16_shadow():
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(0)
    m = torch.nn.Linear(37, 5)
    f = FlatParams(m, shadow_dtype=torch.bfloat16)
    o = SGD(m.parameters(), lr=0.1, momentum=0.9)
    ema = WeightEMA(o, decay=0.5)
    for _ in range(2):
        o.zero_grad()
        for p in m.parameters():
            p.main_grad.copy_(torch.randn(p.shape))
            f.grad_done(p)
        o.step()
    master, buf, shadow = f.master.clone(), ema.buffer.clone(), f.shadow.clone()
    assert torch.equal(shadow, master.to(torch.bfloat16)) and not torch.equal(buf, master)
    with ema.applied():
        assert torch.equal(f.master, buf) and torch.equal(f.shadow, buf.to(torch.bfloat16))
    assert torch.equal(f.master, master) and torch.equal(ema.buffer, buf) and torch.equal(f.shadow, shadow)


def test_argument_errors():
    m, o, ema = _model("sgd", decay=0.9)
    with pytest.raises(ValueError, match="already"):
        WeightEMA(o)
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(every=0), dict(every=1.5)):
        m2 = MLP(hidden=64)
        ddpx.prepare_model(m2, CPU)
        with pytest.raises(ValueError):
            WeightEMA(SGD(m2.parameters(), lr=0.1), **kw)
    with pytest.raises(ValueError):
        WeightEMA(torch.optim.SGD(MLP(hidden=64).parameters(), lr=0.1))


def _cli(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), *extra, "--device", "cpu", "--model", "mlp", "--data",
           "synthetic", "--full_checkpoint",
           # (a small model and data set: the run is about the flags, the prints and the files, and stays quick)
           "--hidden", "128", "--batch_size", "64", "--train_size", "256", "--test_size", "64"]
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)


EMA_LINE = r"EMA model has accuracy=\d+\.\d\d%"


def test_singlegpu_cli_ema_checkpoints_and_resume(tmp_path):
    r = _cli(tmp_path, "1", "1", "--ema_decay", "0.99", "--metrics", "metrics.jsonl")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    records = [json.loads(ln) for ln in open(tmp_path / "metrics.jsonl")]
    assert [rec["ema_updates"] for rec in records if "epoch" in rec] == [4]
    lines = r.stdout.splitlines()
    k = [i for i, ln in enumerate(lines) if re.fullmatch(r"fp32 model has accuracy=\d+\.\d\d%", ln)]
    assert len(k) == 1 and re.fullmatch(EMA_LINE, lines[k[0] + 1]), r.stdout
    plain = torch.load(tmp_path / "checkpoint.pt", weights_only=True)
    avg = torch.load(tmp_path / "checkpoint_ema.pt", weights_only=True)
    assert list(avg) == list(plain)
    assert all(a.shape == plain[n].shape and a.dtype == plain[n].dtype for n, a in avg.items())
    assert any(not torch.equal(a, plain[n]) for n, a in avg.items())
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["extra"]["ema"]
    assert (st["decay"], st["warmup"], st["every"], st["steps"], st["updates"]) == (0.99, False, 1, 4, 4)
    assert all(torch.equal(st["params"][n], avg[n]) for n in st["params"])
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]
    # resume: epoch 1 only, the counts continue from the file
    r = _cli(tmp_path, "2", "1", "--ema_decay", "0.99", "--resume")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[GPU0] Epoch 1 |" in r.stdout and "[GPU0] Epoch 0 |" not in r.stdout and "note:" not in r.stdout, r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["extra"]["ema"]
    assert (st["steps"], st["updates"]) == (8, 8)


def test_singlegpu_cli_without_the_flag_and_resume_without_ema_state(tmp_path):
    r = _cli(tmp_path, "1", "1")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "EMA" not in r.stdout and not os.path.exists(tmp_path / "checkpoint_ema.pt"), r.stdout
    assert torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["extra"] == {}
    # that file under --ema_decay: the average restarts from the loaded weights, with one note
    r = _cli(tmp_path, "2", "1", "--ema_decay", "0.99", "--ema_every", "2", "--resume")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("holds no EMA state") == 1 and re.search(EMA_LINE, r.stdout), r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["extra"]["ema"]
    assert (st["every"], st["steps"], st["updates"]) == (2, 4, 2)
