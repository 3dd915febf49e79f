"""``ddpx.optim.AdamW`` on the CPU path: bit parity with ``torch.optim.AdamW(foreach=False)``, state-dict
interchange with torch in both directions, argument errors, the CLI defaults, DDP (replicated and ZeRO-1) against
torch DDP, and ``singlegpu.py --optimizer adamw`` with a full-checkpoint resume."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests._dist_util import free_port, init_gloo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 1 << 18  # the CPU sweep's block
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


class _Odd(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n) * 0.1) for n in sizes])


def _pair(sizes, seed=0):
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(seed)
    m = _Odd(sizes)
    twin = _Odd(sizes)
    twin.load_state_dict(m.state_dict())
    return m, twin, FlatParams(m)


def _grads(m, twin, flat, t, gen):
    """The same gradient for both models; step 3 is tiny (1e-4 of the others), step 4 has exact zeros."""
    flat.grad.fill_(float("nan"))  # the padding stays NaN: it must never reach a parameter
    for p, q in zip(m.parameters(), twin.parameters()):
        g = torch.randn(p.shape, generator=gen) * (1e-4 if t == 3 else 0.5)
        if t == 4:
            g.view(-1)[::3] = 0
        p.main_grad.copy_(g)
        flat.grad_done(p)
        q.grad = g.clone()


def _assert_same_bits(opt, topt, m, twin, what):
    sd = opt.state_dict()["state"]
    for i, (p, q) in enumerate(zip(m.parameters(), twin.parameters())):
        assert torch.equal(p.detach(), q.detach()), (what, "param", i)
        st = topt.state[q]
        assert torch.equal(sd[i]["exp_avg"], st["exp_avg"]), (what, "exp_avg", i)
        assert torch.equal(sd[i]["exp_avg_sq"], st["exp_avg_sq"]), (what, "exp_avg_sq", i)
        assert float(sd[i]["step"]) == float(st["step"]), (what, "step", i)


def test_cpu_sweep_is_bitwise_torch_adamw():
    """Odd-sized parameters, one of them spanning several blocks of the sweep plus a remainder."""
    from ddpx.optim import AdamW
    sizes = [1, 3, 5, 1023, BLK + 7, 2 * BLK + 13]
    m, twin, flat = _pair(sizes)
    opt = AdamW(m.parameters(), **HP)
    topt = torch.optim.AdamW(twin.parameters(), foreach=False, **HP)
    gen = torch.Generator().manual_seed(1)
    for t in range(1, 6):
        _grads(m, twin, flat, t, gen)
        opt.step()
        topt.step()
        opt.zero_grad()
        _assert_same_bits(opt, topt, m, twin, f"step {t}")
    assert opt.steps_taken() == 5 and flat.fused_opt is None and not opt.fused_active()


def test_state_dict_interchanges_with_torch_both_ways():
    from ddpx.optim import AdamW
    sizes = [1, 3, 65, 700]
    gen = torch.Generator().manual_seed(2)
    # ddpx -> torch
    m, twin, flat = _pair(sizes, seed=3)
    opt = AdamW(m.parameters(), **HP)
    for t in range(1, 4):
        _grads(m, twin, flat, t, gen)
        opt.step()
        opt.zero_grad()
    sd = opt.state_dict()
    keys = ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
            "fused", "decoupled_weight_decay", "params"]
    assert sorted(sd["param_groups"][0]) == sorted(keys) and sd["ddpx_step_count"] == 3
    for i, p in enumerate(m.parameters()):
        s = sd["state"][i]
        assert list(s) == ["step", "exp_avg", "exp_avg_sq"]
        assert s["step"].dtype == torch.float32 and s["step"].dim() == 0 and float(s["step"]) == 3.0
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
    twin.load_state_dict(m.state_dict())
    topt = torch.optim.AdamW(twin.parameters(), foreach=False, lr=1.0)  # every hyper-parameter comes from the file
    topt.load_state_dict({k: v for k, v in sd.items() if k != "ddpx_step_count"})
    for t in (4, 5):
        _grads(m, twin, flat, t, gen)
        opt.step()
        topt.step()
        opt.zero_grad()
    _assert_same_bits(opt, topt, m, twin, "ddpx -> torch")
    # torch -> ddpx
    m, twin, flat = _pair(sizes, seed=4)
    topt = torch.optim.AdamW(twin.parameters(), foreach=False, **HP)
    for t in range(1, 4):
        _grads(m, twin, flat, t, gen)
        topt.step()
    m.load_state_dict(twin.state_dict())
    opt = AdamW(m.parameters(), lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5)
    opt.load_state_dict(topt.state_dict())
    assert opt.steps_taken() == 3 and opt.param_groups[0]["betas"] == HP["betas"]
    for t in (4, 5):
        _grads(m, twin, flat, t, gen)
        opt.step()
        topt.step()
        opt.zero_grad()
    _assert_same_bits(opt, topt, m, twin, "torch -> ddpx")


def test_argument_errors_and_foreign_state():
    from ddpx.optim import SGD, AdamW
    from ddpx.runtime.flat_params import FlatParams

    def prep():
        m = _Odd([4, 70])
        FlatParams(m)
        return m
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW(prep().parameters(), amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        AdamW(prep().parameters(), maximize=True)
    m = prep()
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="single parameter group"):
        AdamW([{"params": ps[:1]}, {"params": ps[1:], "lr": 0.1}])
    with pytest.raises(ValueError):
        AdamW(prep().parameters(), max_grad_norm=0.0)
    with pytest.raises(ValueError):
        AdamW(prep().parameters(), betas=(0.9, 1.0))
    # a state written by the other optimizer is refused, not loaded
    a, s = AdamW(prep().parameters()), SGD(prep().parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match="another optimizer"):
        a.load_state_dict(s.state_dict())
    with pytest.raises(ValueError, match="another optimizer"):
        s.load_state_dict(a.state_dict())


def test_parser_defaults_follow_the_optimizer():
    from ddpx.train.app import build_parser
    a = build_parser("t").parse_args(["1", "1"])
    assert a.optimizer == "sgd" and a.lr == 0.4 and a.weight_decay == 5e-4
    a = build_parser("t").parse_args(["1", "1", "--optimizer", "adamw"])
    assert a.lr == 1e-3 and a.weight_decay == 0.01 and tuple(a.betas) == (0.9, 0.999) and a.eps == 1e-8
    a = build_parser("t").parse_args(["1", "1", "--optimizer", "adamw", "--lr", "0.02", "--betas", "0.8", "0.95",
                                      "--eps", "1e-6", "--weight_decay", "0.1"])
    assert a.lr == 0.02 and tuple(a.betas) == (0.8, 0.95) and a.eps == 1e-6 and a.weight_decay == 0.1
    a = build_parser("t").parse_args(["1", "1", "--lr", "0.2"])
    assert a.lr == 0.2 and a.weight_decay == 5e-4


def test_build_model_and_optimizer_builds_the_chosen_one():
    from ddpx.optim import SGD, AdamW
    from ddpx.train.app import build_model_and_optimizer, build_parser
    common = ["1", "1", "--model", "mlp", "--hidden", "64", "--device", "cpu"]
    args = build_parser("t").parse_args(common + ["--optimizer", "adamw", "--clip_grad_norm", "2.0"])
    _, opt = build_model_and_optimizer(args, torch.device("cpu"))
    g = opt.param_groups[0]
    assert type(opt) is AdamW and g["lr"] == 1e-3 and g["weight_decay"] == 0.01 and opt.max_grad_norm == 2.0
    assert opt.flat.fused_opt is None and set(opt.flat.state_tensors) == {"exp_avg", "exp_avg_sq"}
    _, opt = build_model_and_optimizer(build_parser("t").parse_args(common), torch.device("cpu"))
    g = opt.param_groups[0]
    assert type(opt) is SGD and g["lr"] == 0.4 and g["weight_decay"] == 5e-4 and g["momentum"] == 0.9


def _ddp_worker(rank, ws, port, overlap, shard):
    import ddpx
    from ddpx.models import DeepNN
    from ddpx.optim import AdamW
    from ddpx.parallel.comm import TorchComm
    from ddpx.parallel.ddp import DistributedDataParallel
    from torch.nn.parallel import DistributedDataParallel as TorchDDP
    init_gloo(rank, ws, port)
    try:
        torch.manual_seed(100 + rank)  # replicas start different: DDP init broadcasts rank 0
        ours, ref = DeepNN(), DeepNN()
        ours.classifier[2].p = 0.0
        ref.classifier[2].p = 0.0
        ref.load_state_dict(ours.state_dict())
        ddpx.prepare_model(ours, "cpu")
        # the optimizer first, as the training script builds it: its state must follow the sharded re-layout
        o_ours = AdamW(ours.parameters(), **HP)
        d_ours = DistributedDataParallel(ours, comm=TorchComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                         overlap_optimizer=overlap, shard_optimizer=shard)
        if overlap or shard:
            d_ours.attach_optimizer(o_ours)
        assert d_ours.sharded == shard
        d_ref = TorchDDP(ref, bucket_cap_mb=1.0)
        o_ref = torch.optim.AdamW(ref.parameters(), **HP)
        g = torch.Generator().manual_seed(rank)
        for _ in range(4):
            x = torch.rand((4, 3, 32, 32), generator=g)
            t = torch.randint(0, 10, (4,), generator=g)
            for net, opt in ((d_ours, o_ours), (d_ref, o_ref)):
                opt.zero_grad()
                F.cross_entropy(net(x), t).backward()
                opt.step()
        d_ours.consolidate()
        # tests/test_ddp_cpu.py's DDP tolerance
        for (n, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p, q, atol=2e-5, rtol=1e-4), (rank, n, (p - q).abs().max().item())
        so, sr = o_ours.state_dict()["state"], o_ref.state_dict()["state"]
        for i in sr:
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.allclose(so[i][k], sr[i][k], atol=2e-5, rtol=1e-4), (i, k)
            assert float(so[i]["step"]) == float(sr[i]["step"]) == 4.0
        flat = o_ours.flat.master.clone()
        lst = [torch.empty_like(flat) for _ in range(ws)]
        dist.all_gather(lst, flat)
        assert all(torch.equal(o, lst[0]) for o in lst)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap,shard", [(False, False), (True, False), (False, True)])
def test_ddp_adamw_matches_torch_ddp(overlap, shard):
    mp.spawn(_ddp_worker, args=(2, free_port(), overlap, shard), nprocs=2, join=True)


def _cli(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), *extra, "--device", "cpu", "--model", "mlp", "--data",
           "synthetic", "--full_checkpoint",
           # (a small model and data set: the run is about the flags, the prints and the file, and stays quick)
           "--hidden", "128", "--batch_size", "64", "--train_size", "256", "--test_size", "64"]
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)


def test_singlegpu_cli_adamw_full_checkpoint_resume_and_mismatch(tmp_path):
    r = _cli(tmp_path, "1", "1", "--optimizer", "adamw")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert "[GPU0] Epoch 0 | Batchsize: 64 | Steps: 4" in lines, r.stdout
    assert "Epoch 0 | Training checkpoint saved at checkpoint.pt" in lines, r.stdout
    assert any(re.fullmatch(r"Total training time: \d+\.\d\d seconds", ln) for ln in lines), r.stdout
    assert any(re.fullmatch(r"fp32 model has accuracy=\d+\.\d\d%", ln) for ln in lines), r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["optimizer"]
    assert "betas" in st["param_groups"][0] and float(st["state"][0]["step"]) == 4.0
    assert all(s["exp_avg_sq"].abs().sum() > 0 for s in st["state"].values())
    # resume: epoch 1 only, the step count continues
    r = _cli(tmp_path, "2", "1", "--optimizer", "adamw", "--resume")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[GPU0] Epoch 1 | Batchsize: 64 | Steps: 4" in r.stdout and "[GPU0] Epoch 0 |" not in r.stdout, r.stdout
    st = torch.load(tmp_path / "checkpoint_full.pt", weights_only=True)["optimizer"]
    assert float(st["state"][0]["step"]) == 8.0
    # the AdamW file under --optimizer sgd: a clear error, nothing loaded
    r = _cli(tmp_path, "3", "1", "--resume")
    assert r.returncode != 0 and "another optimizer" in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
