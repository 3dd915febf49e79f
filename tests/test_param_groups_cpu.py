"""Parameter groups of the flat optimizers on the CPU path, which defines their semantics: two-group SGD and AdamW
bitwise against ``torch.optim.SGD`` / ``AdamW(foreach=False)`` with the same groups, LARS and LAMB against the
per-parameter fp64 loops of ``tests/_groups_ref.py`` (bounds: ``tests/_lars_ref.py`` / ``tests/_lamb_ref.py`` with
k = 2, the CPU sweep's mul + add per fma; the CPU path steps with each group's own rate, so no rounding is spent on
forming it), the state dict in torch's multi-group format, the argument errors, ``decay_groups`` and
``singlegpu.py --no_decay_1d``."""
import os
import subprocess
import sys

import pytest
import torch

from tests._groups_ref import LambGroupsFp64, LarsGroupsFp64
from tests._lars_ref import f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#          2-D > one chunk  1-D    2-D      1-D   2-D (does not adapt)  1-D
SHAPES = [(300, 231), (5,), (7, 9), (70,), (6, 11), (1,)]
DECAY = [0, 2, 4]      # group 0: weight decay, the base rate
NO_DECAY = [1, 3, 5]   # group 1: none, a tenth of the rate


class _Mixed(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s) * 0.1) for s in shapes])


def _pair(seed=0, shapes=SHAPES):
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m, twin = _Mixed(shapes), _Mixed(shapes)
    twin.load_state_dict(m.state_dict())
    return m, twin, FlatParams(m)


def _groups(model, lrs, wds=(5e-4, 0.0), **extra):
    ps = list(model.parameters())
    return [{"params": [ps[i] for i in DECAY], "lr": lrs[0], "weight_decay": wds[0]},
            {"params": [ps[i] for i in NO_DECAY], "lr": lrs[1], "weight_decay": wds[1], **extra}]


def _grads(m, twin, flat, gen):
    """The same random gradient for both models (NaN in every padding element of the store)."""
    flat.grad.fill_(float("nan"))
    out = []
    for p, q in zip(m.parameters(), twin.parameters() if twin is not None else m.parameters()):
        g = torch.randn(p.shape, generator=gen) * 0.5
        p.main_grad.copy_(g)
        flat.grad_done(p)
        if twin is not None:
            q.grad = g.clone()
        out.append(g)
    return out


def _lam(k):
    return (k + 1) / 4 if k < 3 else 1.0 - 0.1 * (k - 3)


def _make(kind, m, twin, lrs):
    """(ddpx optimizer over ``m``, torch's over ``twin``) with the same two groups; None for a model not given."""
    from ddpx.optim import SGD, AdamW
    hp = dict(momentum=0.9) if kind == "sgd" else dict(betas=(0.9, 0.999), eps=1e-8)
    cls, tcls = (SGD, torch.optim.SGD) if kind == "sgd" else (AdamW, torch.optim.AdamW)
    return (cls(_groups(m, lrs), lr=9.0, allow_groups=True, **hp) if m is not None else None,
            tcls(_groups(twin, lrs), lr=9.0, foreach=False, **hp) if twin is not None else None)


def _state_keys(kind):
    return ["momentum_buffer"] if kind == "sgd" else ["exp_avg", "exp_avg_sq", "step"]


def _assert_same_bits(kind, opt, topt, m, twin, what):
    """Master and state against torch's, the state read through torch's running index across the groups."""
    sd = opt.state_dict()
    order = [p for g in opt.param_groups for p in g["params"]]
    torder = [q for g in topt.param_groups for q in g["params"]]
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(DECAY), len(NO_DECAY)]
    assert sd["param_groups"][1]["params"] == list(range(len(DECAY), len(SHAPES)))
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach()), (what, "param")
    for i, (p, q) in enumerate(zip(order, torder)):
        for key in _state_keys(kind):
            a, b = sd["state"][i][key], topt.state[q][key]
            assert torch.equal(torch.as_tensor(a).float(), torch.as_tensor(b).float()), (what, key, i)


@pytest.mark.parametrize("kind,lrs", [("sgd", (0.4, 0.04)), ("adamw", (1e-3, 1e-4))])
def test_two_groups_are_bitwise_torch(kind, lrs):
    """wd 5e-4 / 0 and two learning rates under one LambdaLR, 5 steps: master and state bitwise torch's."""
    m, twin, flat = _pair()
    opt, topt = _make(kind, m, twin, lrs)
    assert len(opt.param_groups) == 2 and not opt.fused_active()
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _lam)
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, _lam)
    gen = torch.Generator().manual_seed(1)
    for t in range(5):
        _grads(m, twin, flat, gen)
        opt.sync_lr()  # (checks that the groups kept their ratio)
        opt.step()
        topt.step()
        opt.zero_grad()
        sched.step()
        tsched.step()
        _assert_same_bits(kind, opt, topt, m, twin, f"step {t}")
    h = opt._hyper()
    assert not h.uniform and h.table is None
    assert [h.lr_mul[flat.index[id(p)]] for p in opt.param_groups[1]["params"]] == [f32(lrs[1] / lrs[0])] * 3
    # the padding of the store was never written
    pad = torch.ones(flat.total, dtype=torch.bool)
    for o, n in zip(flat.offsets, flat.numels):
        pad[o:o + n] = False
    assert (flat.master[pad] == 0).all()


@pytest.mark.parametrize("kind,lrs", [("sgd", (0.4, 0.04)), ("adamw", (1e-3, 1e-4))])
def test_state_dict_interchanges_with_torch_both_ways(kind, lrs):
    gen = torch.Generator().manual_seed(2)
    # ddpx -> torch
    m, twin, flat = _pair(seed=3)
    opt, _ = _make(kind, m, None, lrs)
    for _ in range(3):
        _grads(m, twin, flat, gen)
        opt.step()
        opt.zero_grad()
    sd = opt.state_dict()
    twin.load_state_dict(m.state_dict())
    _, topt = _make(kind, None, twin, (7.0, 7.0))  # every hyper-parameter comes from the file
    topt.load_state_dict({k: v for k, v in sd.items() if k != "ddpx_step_count"})
    assert [g["lr"] for g in topt.param_groups] == list(lrs)
    for _ in range(2):
        _grads(m, twin, flat, gen)
        opt.step()
        topt.step()
        opt.zero_grad()
    _assert_same_bits(kind, opt, topt, m, twin, "ddpx -> torch")
    # torch -> ddpx
    m, twin, flat = _pair(seed=4)
    _, topt = _make(kind, None, twin, lrs)
    for _ in range(3):
        _grads(m, twin, flat, gen)
        topt.step()
    m.load_state_dict(twin.state_dict())
    opt, _ = _make(kind, m, None, (7.0, 7.0))
    opt.load_state_dict(topt.state_dict())
    assert [g["lr"] for g in opt.param_groups] == list(lrs) and [g["weight_decay"] for g in opt.param_groups] == [
        5e-4, 0.0]
    for _ in range(2):
        _grads(m, twin, flat, gen)
        opt.step()
        topt.step()
        opt.zero_grad()
    _assert_same_bits(kind, opt, topt, m, twin, "torch -> ddpx")
    # another group structure is refused
    m2, _, _ = _pair(seed=5)
    one = type(opt)(m2.parameters(), lr=lrs[0])
    with pytest.raises(ValueError, match="groups"):
        one.load_state_dict(sd)
    with pytest.raises(ValueError, match="groups"):
        opt.load_state_dict(one.state_dict())


def test_argument_errors():
    from ddpx.optim import LAMB, LARS, SGD, AdamW
    ps = lambda: list(_pair()[0].parameters())  # noqa: E731

    def two(p, **second):
        return [{"params": p[:3]}, {"params": p[3:], **second}]
    # several groups are an explicit choice
    for cls in (SGD, AdamW, LARS, LAMB):
        with pytest.raises(ValueError, match="allow_groups=True"):
            cls(two(ps(), lr=0.1), lr=0.01)
    with pytest.raises(ValueError, match="momentum"):
        SGD(two(ps(), momentum=0.5), allow_groups=True, lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match="nesterov"):
        SGD(two(ps(), nesterov=True), allow_groups=True, lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match="betas"):
        AdamW(two(ps(), betas=(0.8, 0.999)), allow_groups=True)
    with pytest.raises(ValueError, match="eps"):
        LAMB(two(ps(), eps=1e-3), allow_groups=True)
    with pytest.raises(ValueError, match="trust_coef"):
        LARS(two(ps(), trust_coef=0.5), allow_groups=True, lr=0.1)
    # group 0's base rate is 0 and another group's differs: no multiple of it
    for cls in (SGD, AdamW, LARS, LAMB):
        with pytest.raises(ValueError, match="base learning rate is 0"):
            cls(two(ps(), lr=0.1), allow_groups=True, lr=0.0)
        assert len(cls(two(ps(), lr=0.0), allow_groups=True, lr=0.0).param_groups) == 2  # (all zero: equal groups)
    # the groups must own the whole store, once
    p = ps()
    with pytest.raises(ValueError, match="one FlatParams store"):
        SGD([{"params": p[:3]}, {"params": p[4:]}], allow_groups=True, lr=0.1)
    # a broken ratio is reported by sync_lr(), where the host rate goes to the device
    opt = SGD(two(ps(), lr=0.04), allow_groups=True, lr=0.4, momentum=0.9)
    opt.sync_lr()
    opt.param_groups[0]["lr"] = 0.8  # without a scheduler the current rates are the base rates: a new ratio
    opt.sync_lr()
    assert min(opt._hyper().lr_mul) == f32(0.04 / 0.8)
    opt.param_groups[0]["lr"] = 0.4
    torch.optim.lr_scheduler.LambdaLR(opt, _lam)  # (sets every group's initial_lr, and lr = initial_lr / 4)
    opt.sync_lr()
    opt.param_groups[0]["lr"] = 0.2
    with pytest.raises(ValueError, match="ratio"):
        opt.sync_lr()
    opt.param_groups[1]["lr"] = 0.02
    opt.sync_lr()
    # equal groups are one group: the default path, and the fused backward stays available to it
    h = SGD(two(ps()), allow_groups=True, lr=0.1, momentum=0.9, weight_decay=1e-3)._hyper()
    assert h.uniform and h.table is None


def test_decay_groups():
    from ddpx.models import MLP
    from ddpx.optim import decay_groups
    model = MLP(hidden=32)
    g = decay_groups(model, 5e-4)
    assert [sorted(x) for x in g] == [["params", "weight_decay"]] * 2
    assert g[0]["weight_decay"] == 5e-4 and g[1]["weight_decay"] == 0.0
    assert all(p.dim() > 1 for p in g[0]["params"]) and all(p.dim() <= 1 for p in g[1]["params"])
    assert len(g[0]["params"]) + len(g[1]["params"]) == len(list(model.parameters())) and g[1]["params"]


#                  group 1:  lr / 10, no weight decay;                   ... and it does not adapt either
@pytest.mark.parametrize("second", [dict(), dict(adapt=False), dict(exclude_1d=False)],
                         ids=["wd_lr", "adapt_off", "adapt_1d"])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_lars_groups_match_an_independent_fp64_loop(max_norm, second):
    from ddpx.optim import LARS
    m, _, flat = _pair()
    params = list(m.parameters())
    lrs = (0.4, 0.04)
    hp = dict(momentum=0.9, trust_coef=1e-3, eps=1e-8)
    opt = LARS(_groups(m, lrs, **second), lr=9.0, max_grad_norm=max_norm, allow_groups=True, **hp)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _lam)
    grp = [0 if i in DECAY else 1 for i in range(len(SHAPES))]
    ex = [True if g == 0 else second.get("exclude_1d", True) for g in grp]
    adapt = [(g == 0 or second.get("adapt", True)) and (p.dim() > 1 or not e) for g, p, e in zip(grp, params, ex)]
    ref = LarsGroupsFp64(params, [lrs[g] for g in grp], [(5e-4, 0.0)[g] for g in grp], adapt, exclude_1d=False,
                         max_grad_norm=max_norm, k=2, **hp)
    gen = torch.Generator().manual_seed(1)
    for step in range(5):
        grads = _grads(m, None, flat, gen)
        opt.sync_lr()
        opt.step()
        opt.zero_grad()
        ref.step(grads, lr=[f32(opt.param_groups[g]["lr"]) for g in grp])
        sched.step()
        trust = opt.trust_ratio_dev.tolist()
        for i, p in enumerate(params):
            t = trust[flat.index[id(p)]]
            if adapt[i]:
                assert t != 1.0 and abs(t - ref.trust[i]) <= 1e-5 * ref.trust[i], (step, i, t, ref.trust[i])
            else:
                assert t == 1.0, (step, i, t)
    worst = [0.0, 0.0]
    for i, p in enumerate(params):
        buf = opt.momentum_buffer[flat.slice(flat.index[id(p)])]
        worst = [max(a, b) for a, b in zip(worst, ref.check(i, p, buf, "5 cpu steps"))]
    print(f"LARS groups {second} max_norm {max_norm}: achieved fraction of the bound: param {worst[0]:.3f} "
          f"momentum {worst[1]:.3f}")


@pytest.mark.parametrize("second", [dict(), dict(adapt=False), dict(exclude_1d=False)],
                         ids=["wd_lr", "adapt_off", "adapt_1d"])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_lamb_groups_match_an_independent_fp64_loop(max_norm, second):
    from ddpx.optim import LAMB
    m, _, flat = _pair()
    params = list(m.parameters())
    lrs, wds = (1e-2, 1e-3), (0.01, 0.0)
    hp = dict(betas=(0.9, 0.999), eps=1e-6)
    opt = LAMB(_groups(m, lrs, wds, **second), lr=9.0, max_grad_norm=max_norm, allow_groups=True, **hp)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _lam)
    grp = [0 if i in DECAY else 1 for i in range(len(SHAPES))]
    ex = [True if g == 0 else second.get("exclude_1d", True) for g in grp]
    adapt = [(g == 0 or second.get("adapt", True)) and (p.dim() > 1 or not e) for g, p, e in zip(grp, params, ex)]
    ref = LambGroupsFp64(params, [lrs[g] for g in grp], [wds[g] for g in grp], adapt, exclude_1d=False,
                         max_grad_norm=max_norm, k=2, **hp)
    gen = torch.Generator().manual_seed(1)
    for step in range(5):
        grads = _grads(m, None, flat, gen)
        opt.sync_lr()
        opt.step()
        opt.zero_grad()
        ref.step(grads, lr=[f32(opt.param_groups[g]["lr"]) for g in grp])
        sched.step()
        trust = opt.trust_ratio_dev.tolist()
        for i, p in enumerate(params):
            t = trust[flat.index[id(p)]]
            if adapt[i]:
                assert t != 1.0 and abs(t - ref.trust[i]) <= 1e-5 * ref.trust[i], (step, i, t, ref.trust[i])
            else:
                assert t == 1.0, (step, i, t)
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(params):
        sl = flat.slice(flat.index[id(p)])
        worst = [max(a, b) for a, b in zip(worst, ref.check(i, p, opt.exp_avg[sl], opt.exp_avg_sq[sl], "5 cpu steps"))]
    print(f"LAMB groups {second} max_norm {max_norm}: achieved fraction of the bound: param {worst[0]:.3f} "
          f"exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


@pytest.mark.parametrize("name", ["LARS", "LAMB"])
def test_lars_lamb_state_dict_round_trips_the_groups(name):
    import ddpx.optim
    cls = getattr(ddpx.optim, name)
    m, _, flat = _pair(seed=6)
    opt = cls(_groups(m, (0.1, 0.01), adapt=False), lr=9.0, allow_groups=True)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        _grads(m, None, flat, gen)
        opt.step()
        opt.zero_grad()
    sd = opt.state_dict()
    assert sd["param_groups"][1]["adapt"] is False and "adapt" not in sd["param_groups"][0]
    m2, _, _ = _pair(seed=6)
    other = cls(_groups(m2, (7.0, 7.0)), lr=9.0, allow_groups=True)
    other.load_state_dict(sd)
    assert [g["lr"] for g in other.param_groups] == [0.1, 0.01] and other.param_groups[1]["adapt"] is False
    assert other._plain() == opt._plain()
    a, b = other.state_dict()["state"], sd["state"]
    assert all(torch.equal(torch.as_tensor(a[i][k]), torch.as_tensor(b[i][k])) for i in b for k in b[i])


@pytest.mark.parametrize("optimizer", ["sgd", "adamw", "lars", "lamb"])
def test_singlegpu_cli_no_decay_1d(tmp_path, optimizer):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--device", "cpu", "--model", "mlp",
           "--no_decay_1d", "--optimizer", optimizer, "--data", "synthetic", "--full_checkpoint",
           # (a small model and data set: the run is about the flag and the file, and stays quick)
           "--hidden", "64", "--batch_size", "64", "--train_size", "128", "--test_size", "64"]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[GPU0] Epoch 0 | Batchsize: 64 | Steps: 2" in r.stdout.splitlines(), r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["optimizer"]
    groups = st["param_groups"]
    assert len(groups) == 2 and groups[0]["weight_decay"] > 0 and groups[1]["weight_decay"] == 0.0
    assert groups[1]["params"][0] == len(groups[0]["params"]) and len(st["state"]) == sum(
        len(g["params"]) for g in groups)
    # the two-group file resumes; under one group it is refused
    r = subprocess.run(cmd[:2] + ["2", "1"] + cmd[4:] + ["--resume"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "[GPU0] Epoch 1 |" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    if optimizer == "sgd":
        one = [c for c in cmd[:2] + ["3", "1"] + cmd[4:] + ["--resume"] if c != "--no_decay_1d"]
        r = subprocess.run(one, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "groups" in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
