"""``ddpx.optim.LAMB`` on the CPU path: an independent per-parameter fp64 loop, ``torch.optim.AdamW`` where every
trust ratio is 1, the state dict, foreign states, DDP (replicated and ZeRO-1) against a single process on the
concatenated batch, and ``singlegpu.py --optimizer lamb`` with a full-checkpoint resume.

The bound of the fp64 comparisons is ``tests/_lamb_ref.py``'s accumulation with k = 2: the CPU sweep spends a mul
and an add where the kernels have one fma.  The achieved fractions are printed."""
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo
from tests._lamb_ref import LambFp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
#          1-D       2-D      2-D zero weights  2-D zero gradient  2-D no gradient  2-D > one chunk  1-D
SHAPES = [(5,), (7, 9), (6, 11), (4, 17), (3, 5), (300, 231), (70,)]
ZERO_W, ZERO_G, NO_G = 2, 3, 4


class _Mixed(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s) * 0.1) for s in shapes])


def _model(shapes, seed=0):
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m = _Mixed(shapes)
    with torch.no_grad():
        if len(shapes) == len(SHAPES):
            m.ps[ZERO_W].zero_()
    return m, FlatParams(m)


def _grads(m, flat, gen, special=True):
    """Random gradients into the store (NaN in every padding element); returns them per parameter, None for the
    parameter nobody produced a gradient for."""
    flat.grad.fill_(float("nan"))
    out = []
    for i, p in enumerate(m.parameters()):
        if special and i == NO_G:
            out.append(None)
            continue
        g = torch.randn(p.shape, generator=gen) * 0.5
        if special and i == ZERO_G:
            g.zero_()
        p.main_grad.copy_(g)
        flat.grad_done(p)
        out.append(g)
    return out


def _states(opt, flat, p):
    sl = flat.slice(flat.index[id(p)])
    return opt.exp_avg[sl], opt.exp_avg_sq[sl]


@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_five_steps_match_an_independent_fp64_loop(max_norm):
    from ddpx.optim import LAMB
    m, flat = _model(SHAPES)
    params = list(m.parameters())
    opt = LAMB(params, max_grad_norm=max_norm, **HP)
    ref = LambFp64(params, max_grad_norm=max_norm, k=2, **HP)
    untouched = params[NO_G].detach().clone()
    gen = torch.Generator().manual_seed(1)
    for step in range(5):
        grads = _grads(m, flat, gen)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "parameters without gradient this step"
            opt.step()
        opt.zero_grad()
        ref.step(grads)
        trust = opt.trust_ratio_dev.tolist()
        for i, p in enumerate(params):
            j = flat.index[id(p)]
            # a zero gradient with zero moments and zero weights gives u = 0; the zero weights stay zero under
            # LAMB while wn = 0 (t = 1, u = r + wd 0): after step 0 they have moved and adapt.  A zero gradient
            # alone does not make u zero (weight decay), so ZERO_G adapts.
            if p.dim() <= 1 or i == NO_G or (i == ZERO_W and step == 0):
                assert trust[j] == 1.0, (step, i, trust[j])
            else:
                assert trust[j] != 1.0 and abs(trust[j] - ref.trust[i]) <= 1e-5 * ref.trust[i], (step, i)
        if max_norm is not None:
            assert ref.norm > 2 * max_norm, "the clip must be active"
            assert abs(opt.grad_norm_dev.item() - ref.norm) <= 1e-6 * ref.norm
            assert abs(opt.clip_coef_dev.item() - ref.coef) <= 1e-6 * ref.coef
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(params):
        mm, vv = _states(opt, flat, p)
        worst = [max(a, b) for a, b in zip(worst, ref.check(i, p, mm, vv, "5 cpu steps"))]
    print(f"5 CPU steps (max_norm {max_norm}): achieved fraction of the bound: param {worst[0]:.3f} "
          f"exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")
    assert opt.steps_taken() == 5
    assert torch.equal(params[NO_G].detach(), untouched)  # no gradient: no weight decay, no moments
    mm, vv = _states(opt, flat, params[NO_G])
    assert (mm == 0).all() and (vv == 0).all()
    assert (opt.grad_norm_dev is None) == (max_norm is None)
    assert flat.fused_opt is None and not opt.fused_active()
    # the padding of the store was never written
    pad = torch.ones(flat.total, dtype=torch.bool)
    for o, n in zip(flat.offsets, flat.numels):
        pad[o:o + n] = False
    assert (flat.master[pad] == 0).all() and (opt.exp_avg[pad] == 0).all() and (opt.exp_avg_sq[pad] == 0).all()


def test_all_parameters_1d_tracks_torch_adamw_in_fp64():
    """Every ratio is 1: the update is AdamW's in non-decoupled form, w - lr (r + wd w) against torch's
    w (1 - lr wd) - lr r: mathematically equal.  torch.optim.AdamW runs on fp64 copies (with the hyper-parameters
    the reference rounds to fp32 taken as torch takes them: the difference is below the bound's first rounding)."""
    from ddpx.ops.clip import CHUNK
    from ddpx.optim import LAMB
    shapes = [(1,), (3,), (65,), (CHUNK + 5,)]
    a, fa = _model(shapes, seed=3)
    params = list(a.parameters())
    opt = LAMB(params, **HP)
    ref = LambFp64(params, k=2, **HP)
    twins = [torch.nn.Parameter(p.detach().double().clone()) for p in params]
    tw = torch.optim.AdamW(twins, lr=ref.lr, betas=HP["betas"], eps=ref.eps, weight_decay=ref.wd)
    for step in range(5):
        grads = _grads(a, fa, torch.Generator().manual_seed(10 + step), special=False)
        opt.step()
        ref.step(grads)
        for q, g in zip(twins, grads):
            q.grad = g.double()
        tw.step()
        assert (opt.trust_ratio_dev == 1).all()
    worst = 0.0
    for i, (p, q) in enumerate(zip(params, twins)):
        # the reference itself against torch in fp64: the same mathematics (w1, b2, w2 and the bias corrections
        # rounded to fp32 in the reference: relative 2^-24 each, inside the bound's first terms)
        bound = ref.Ep[i] + 2.0 ** -149
        frac = ((p.detach().double() - q.detach()).abs() / bound).max().item()
        worst = max(worst, frac)
        assert frac <= 1.0, (i, frac)
    print(f"5 CPU steps, all ratios 1, against torch.optim.AdamW in fp64: achieved fraction of the bound {worst:.3f}")
    # with the exclusion off the same store takes trust ratios
    c, fc = _model(shapes, seed=3)
    oc = LAMB(c.parameters(), exclude_1d=False, **HP)
    _grads(c, fc, torch.Generator().manual_seed(10), special=False)
    oc.step()
    assert (oc.trust_ratio_dev != 1).all()


def test_state_dict_round_trip_and_foreign_states():
    from ddpx.optim import LAMB, LARS, SGD, AdamW
    a, fa = _model(SHAPES, seed=6)
    oa = LAMB(a.parameters(), **HP)
    for step in range(3):
        _grads(a, fa, torch.Generator().manual_seed(20 + step), special=False)
        oa.step()
    sd = oa.state_dict()
    g0 = sd["param_groups"][0]
    adamw_keys = set(AdamW(_model(SHAPES)[0].parameters()).state_dict()["param_groups"][0])
    assert set(g0) == adamw_keys | {"exclude_1d"}
    assert g0["eps"] == 1e-6 and g0["exclude_1d"] is True and sd["ddpx_step_count"] == 3
    for i, p in enumerate(a.parameters()):
        assert sorted(sd["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert sd["state"][i]["exp_avg"].shape == p.shape and float(sd["state"][i]["step"]) == 3.0
    # a fresh optimizer with other hyper-parameters takes everything from the state and continues bit for bit
    b, fb = _model(SHAPES, seed=7)
    b.load_state_dict(a.state_dict())
    ob = LAMB(b.parameters(), lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.1, exclude_1d=False)
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["exclude_1d"] is True and ob.param_groups[0]["betas"] == (0.9, 0.999)
    assert ob.steps_taken() == 3
    for step in (3, 4):
        for m, f in ((a, fa), (b, fb)):
            _grads(m, f, torch.Generator().manual_seed(20 + step), special=False)
        oa.step()
        ob.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p.detach(), q.detach())
    assert torch.equal(oa.trust_ratio_dev, ob.trust_ratio_dev) and (oa.trust_ratio_dev != 1).any()
    # foreign states, both ways
    s = SGD(_model(SHAPES)[0].parameters(), lr=0.1, momentum=0.9)
    w = AdamW(_model(SHAPES)[0].parameters())
    r = LARS(_model(SHAPES)[0].parameters(), lr=0.1)
    for other in (s, w, r):
        with pytest.raises(ValueError, match="another optimizer"):
            ob.load_state_dict(other.state_dict())
        with pytest.raises(ValueError, match="another optimizer"):
            other.load_state_dict(sd)


def test_argument_errors_and_cli_defaults():
    from ddpx.optim import LAMB
    from ddpx.train.app import build_model_and_optimizer, build_parser
    for bad in (dict(max_grad_norm=0.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-1.0),
                dict(lr=-1.0)):
        with pytest.raises(ValueError):
            LAMB(_model([(4,), (3, 3)])[0].parameters(), **bad)
    ps = list(_model([(4,), (3, 3)])[0].parameters())
    with pytest.raises(ValueError, match="single parameter group"):
        LAMB([{"params": ps[:1]}, {"params": ps[1:], "lr": 0.1}])
    a = build_parser("t").parse_args(["1", "1", "--optimizer", "lamb"])
    assert a.lr == 1e-3 and a.weight_decay == 0.01 and a.eps == 1e-6 and tuple(a.betas) == (0.9, 0.999)
    # the other optimizers' defaults are unchanged
    a = build_parser("t").parse_args(["1", "1"])
    assert a.optimizer == "sgd" and a.lr == 0.4 and a.weight_decay == 5e-4 and a.eps == 1e-8
    a = build_parser("t").parse_args(["1", "1", "--optimizer", "adamw"])
    assert a.lr == 1e-3 and a.weight_decay == 0.01 and a.eps == 1e-8
    a = build_parser("t").parse_args(["1", "1", "--optimizer", "lars"])
    assert a.lr == 0.4 and a.weight_decay == 5e-4 and a.trust_coef == 1e-3 and a.lars_eps == 1e-8
    args = build_parser("t").parse_args(["1", "1", "--model", "mlp", "--hidden", "64", "--device", "cpu", "--optimizer",
                                         "lamb", "--betas", "0.8", "0.99", "--eps", "1e-5", "--clip_grad_norm",
                                         "2.0"])
    _, opt = build_model_and_optimizer(args, torch.device("cpu"))
    g = opt.param_groups[0]
    assert type(opt) is LAMB and g["lr"] == 1e-3 and g["weight_decay"] == 0.01 and g["betas"] == (0.8, 0.99)
    assert g["eps"] == 1e-5 and g["exclude_1d"] is True and opt.max_grad_norm == 2.0
    assert opt.flat.fused_opt is None and set(opt.flat.state_tensors) == {"exp_avg", "exp_avg_sq"}


def test_plan_errors():
    from ddpx.ops.lamb import LambPlan, bias_corrections
    m, flat = _model(SHAPES, seed=2)
    _grads(m, flat, torch.Generator().manual_seed(3), special=False)
    mm, vv = torch.zeros_like(flat.master), torch.zeros_like(flat.master)
    bc = bias_corrections(1, 0.9, 0.999)
    plan = LambPlan(flat)
    plan.compute(mm, vv, bc, (0.9, 0.999), 1e-6, 0.01)
    with pytest.raises(ValueError, match="cuts the chunk"):
        plan.apply(flat.offsets[5] + 8, flat.total, 1e-3, mm, vv, bc, 1e-6, 0.01)
    half = LambPlan(flat, [(0, flat.offsets[5])])
    with pytest.raises(ValueError, match="cover"):
        half.apply(0, flat.total, 1e-3, mm, vv, bc, 1e-6, 0.01)
    with pytest.raises(ValueError, match="numel"):
        plan.apply(0, flat.total, 1e-3, mm[:-8], vv, bc, 1e-6, 0.01)
    with pytest.raises(ValueError, match="numel"):
        plan.moments(0, mm, vv[:-8], bc, (0.9, 0.999), 1e-6, 0.01)
    with pytest.raises(ValueError, match="bias corrections"):
        plan.apply(0, flat.total, 1e-3, mm, vv, None, 1e-6, 0.01)
    with pytest.raises(ValueError):
        LambPlan(flat, [(0, flat.total + 8)])


def _ddp_worker(rank, ws, port, overlap, shard, max_norm):
    import ddpx
    from ddpx.models import MLP
    from ddpx.optim import LAMB
    from ddpx.parallel.comm import TorchComm
    from ddpx.parallel.ddp import DistributedDataParallel
    init_gloo(rank, ws, port)
    try:
        hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=max_norm)
        torch.manual_seed(100 + rank)  # replicas start different: DDP init broadcasts rank 0
        ours = MLP(hidden=64)
        torch.manual_seed(100)
        single = MLP(hidden=64)  # rank 0's init
        ddpx.prepare_model(ours, "cpu")
        ddpx.prepare_model(single, "cpu")
        # the optimizer first, as the training script builds it: its state must follow the sharded re-layout
        o = LAMB(ours.parameters(), **hp)
        d = DistributedDataParallel(ours, comm=TorchComm(), bucket_cap_mb=0.5, first_bucket_mb=0.25,
                                    overlap_optimizer=overlap, shard_optimizer=shard)
        if overlap or shard:
            d.attach_optimizer(o)
        assert d.sharded == shard
        if shard:
            f = o.flat
            split = False
            for b in range(len(d.bucket_ranges)):
                if d.bucket_modes[b] == 1:
                    cut = d.bucket_ranges[b][0] + (d.bucket_ranges[b][1] - d.bucket_ranges[b][0]) // ws
                    split |= any(off < cut < off + n for off, n in zip(f.offsets, f.numels))
            assert split, "a parameter must be split across the two shards"
        o1 = LAMB(single.parameters(), **hp)
        B = 8
        for s in range(4):
            g = torch.Generator().manual_seed(1000 + s)
            x = torch.rand(ws * B, 3072, generator=g)
            t = torch.randint(0, 10, (ws * B,), generator=g)
            o.zero_grad()
            loss, _ = d.forward_loss(x[rank * B:(rank + 1) * B], t[rank * B:(rank + 1) * B])
            loss.backward()
            o.step()
            o1.zero_grad()
            l1, _ = single.forward_loss(x, t)
            l1.backward()
            o1.step()
            mine = o.trust_ratio_dev.clone()
            both = [torch.empty_like(mine) for _ in range(ws)]
            dist.all_gather(both, mine)
            assert all(torch.equal(b, both[0]) for b in both), both
            # store orders differ after a sharded re-layout: compare by parameter
            f, f1 = o.flat, o1.flat
            for (n, p), (_, q) in zip(ours.named_parameters(), single.named_parameters()):
                a, b = mine[f.index[id(p)]].item(), o1.trust_ratio_dev[f1.index[id(q)]].item()
                assert (a == 1.0) == (p.dim() <= 1) and abs(a - b) <= 1e-4 * b, (rank, s, n, a, b)
            if max_norm is not None:
                assert o1.clip_coef_dev.item() < 1.0, "the clip must be active"
                assert abs(o.grad_norm_dev.item() - o1.grad_norm_dev.item()) <= 1e-5 * o1.grad_norm_dev.item()
        assert o.steps_taken() == 4
        d.consolidate()
        # tests/test_ddp_cpu.py's DDP tolerance
        for (n, p), (_, q) in zip(ours.named_parameters(), single.named_parameters()):
            assert torch.allclose(p, q, atol=2e-5, rtol=1e-4), (rank, n, (p - q).abs().max().item())
        so, s1 = o.state_dict()["state"], o1.state_dict()["state"]
        for i in s1:
            assert torch.allclose(so[i]["exp_avg"], s1[i]["exp_avg"], atol=2e-5, rtol=1e-4), i
            assert torch.allclose(so[i]["exp_avg_sq"], s1[i]["exp_avg_sq"], atol=2e-5, rtol=1e-4), i
        flat = o.flat.master.clone()
        lst = [torch.empty_like(flat) for _ in range(ws)]
        dist.all_gather(lst, flat)
        assert all(torch.equal(x_, lst[0]) for x_ in lst)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("max_norm", [None, 0.05], ids=["noclip", "clip"])
@pytest.mark.parametrize("overlap,shard", [(False, False), (True, False), (False, True)],
                         ids=["replicated", "overlap", "zero1"])
def test_ddp_lamb_matches_a_single_process(overlap, shard, max_norm):
    mp.spawn(_ddp_worker, args=(2, free_port(), overlap, shard, max_norm), nprocs=2, join=True)


def _cli(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), *extra, "--device", "cpu", "--model", "mlp", "--data",
           "synthetic", "--full_checkpoint",
           # (a small model and data set: the run is about the flags, the prints and the file, and stays quick)
           "--hidden", "128", "--batch_size", "64", "--train_size", "256", "--test_size", "64"]
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)


def test_singlegpu_cli_lamb_full_checkpoint_resume_and_mismatch(tmp_path):
    r = _cli(tmp_path, "1", "1", "--optimizer", "lamb")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert "[GPU0] Epoch 0 | Batchsize: 64 | Steps: 4" in lines, r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["optimizer"]
    assert st["param_groups"][0]["exclude_1d"] is True and st["param_groups"][0]["eps"] == 1e-6
    assert st["ddpx_step_count"] == 4
    assert all(s["exp_avg_sq"].abs().sum() > 0 and float(s["step"]) == 4 for s in st["state"].values())
    # resume: epoch 1 only, the step count continues
    r = _cli(tmp_path, "2", "1", "--optimizer", "lamb", "--resume")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[GPU0] Epoch 1 | Batchsize: 64 | Steps: 4" in r.stdout and "[GPU0] Epoch 0 |" not in r.stdout, r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["optimizer"]
    assert st["ddpx_step_count"] == 8
    # the LAMB file under --optimizer adamw and under --optimizer sgd: a clear error, nothing loaded
    for other in (["--optimizer", "adamw"], []):
        r = _cli(tmp_path, "3", "1", *other, "--resume")
        assert r.returncode != 0 and "another optimizer" in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
