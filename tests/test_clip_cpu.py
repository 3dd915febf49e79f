"""Gradient clipping by global norm (``SGD(max_grad_norm=...)``, ``--clip_grad_norm``) on the CPU path:
DDP semantics against torch DDP + ``clip_grad_norm_`` + ``torch.optim.SGD``, the chunk-table builder, the CLI."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests._dist_util import free_port, init_gloo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ddp_worker(rank, ws, port, overlap, shard, max_norm):
    import ddpx
    from ddpx.models import DeepNN
    from ddpx.optim.sgd import SGD
    from ddpx.parallel.comm import TorchComm
    from ddpx.parallel.ddp import DistributedDataParallel
    from torch.nn.parallel import DistributedDataParallel as TorchDDP
    init_gloo(rank, ws, port)
    try:
        torch.manual_seed(100 + rank)
        ours, ref = DeepNN(), DeepNN()
        ours.classifier[2].p = 0.0
        ref.classifier[2].p = 0.0
        ref.load_state_dict(ours.state_dict())
        ddpx.prepare_model(ours, "cpu")
        d_ours = DistributedDataParallel(ours, comm=TorchComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                         overlap_optimizer=overlap, shard_optimizer=shard)
        d_ref = TorchDDP(ref, bucket_cap_mb=1.0)
        o_ours = SGD(ours.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
        if overlap:
            d_ours.attach_optimizer(o_ours)
        o_ref = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        g = torch.Generator().manual_seed(rank)
        clipped = 0
        for _ in range(3):
            x = torch.rand((4, 3, 32, 32), generator=g)
            t = torch.randint(0, 10, (4,), generator=g)
            o_ours.zero_grad()
            F.cross_entropy(d_ours(x), t).backward()
            o_ours.step()
            o_ref.zero_grad()
            F.cross_entropy(d_ref(x), t).backward()
            tn = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
            o_ref.step()
            clipped += int(tn.item() > max_norm)
            # fp32 gradients summed in another order than torch's per-tensor norms: a few fp32 ulps
            assert abs(o_ours.grad_norm_dev.item() - tn.item()) <= 1e-5 * tn.item(), (o_ours.grad_norm_dev, tn)
            both = [torch.empty(1) for _ in range(ws)]
            dist.all_gather(both, o_ours.grad_norm_dev.reshape(1).clone())
            assert all(torch.equal(b, both[0]) for b in both), both
        assert clipped == 3, "max_norm must be below the gradient norm for this test to bite"
        d_ours.consolidate()
        for (n, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p, q, atol=2e-5, rtol=1e-4), (rank, n, (p - q).abs().max().item())
        so, sr = o_ours.state_dict()["state"], o_ref.state_dict()["state"]
        for i in sr:
            assert torch.allclose(so[i]["momentum_buffer"], sr[i]["momentum_buffer"], atol=2e-5, rtol=1e-4), i
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap,shard", [(True, False), (False, True), (True, True)])
def test_ddp_clip_matches_torch_ddp(overlap, shard):
    mp.spawn(_ddp_worker, args=(2, free_port(), overlap, shard, 0.05), nprocs=2, join=True)


def _no_sync_worker(rank, ws, port):
    import ddpx
    from ddpx.models import DeepNN
    from ddpx.optim.sgd import SGD
    from ddpx.parallel.comm import TorchComm
    from ddpx.parallel.ddp import DistributedDataParallel
    init_gloo(rank, ws, port)
    try:
        torch.manual_seed(0)
        m = DeepNN()
        m.classifier[2].p = 0.0
        single = DeepNN()
        single.classifier[2].p = 0.0
        single.load_state_dict(m.state_dict())
        ddpx.prepare_model(m, "cpu")
        d = DistributedDataParallel(m, comm=TorchComm())
        opt = SGD(m.parameters(), lr=0.1, max_grad_norm=0.05)
        xs = [torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(10 * r + k))
              for r in range(ws) for k in range(2)]
        ts = [torch.randint(0, 10, (2,), generator=torch.Generator().manual_seed(10 * r + k + 5))
              for r in range(ws) for k in range(2)]
        opt.zero_grad()
        with d.no_sync():
            F.cross_entropy(d(xs[2 * rank]), ts[2 * rank]).backward()
        F.cross_entropy(d(xs[2 * rank + 1]), ts[2 * rank + 1]).backward()
        opt.step()
        so = torch.optim.SGD(single.parameters(), lr=0.1)
        so.zero_grad()
        (sum(F.cross_entropy(single(x), t) for x, t in zip(xs, ts)) / ws).backward()
        tn = torch.nn.utils.clip_grad_norm_(single.parameters(), 0.05)
        so.step()
        assert tn.item() > 0.05
        assert abs(opt.grad_norm_dev.item() - tn.item()) <= 1e-5 * tn.item()
        for p, q in zip(m.parameters(), single.parameters()):
            assert torch.allclose(p, q, atol=1e-5, rtol=1e-4)
    finally:
        dist.destroy_process_group()


def test_ddp_no_sync_accumulation_then_clipped_step():
    mp.spawn(_no_sync_worker, args=(2, free_port()), nprocs=2, join=True)


def test_singlegpu_cli_clip_grad_norm_cpu(tmp_path):
    out = tmp_path / "m.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--model", "mlp", "--device", "cpu",
           "--data", "synthetic", "--clip_grad_norm", "1.0", "--metrics", str(out),
           # (a small model and data set: the run is about the flag and the record, and stays quick)
           "--hidden", "128", "--batch_size", "64", "--train_size", "256", "--test_size", "64"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    recs = [json.loads(ln) for ln in out.read_text().splitlines() if ln.strip()]
    steps = [rec for rec in recs if "loss" in rec]  # the per-epoch records (the file ends with a "done" event)
    gn = steps[-1]["grad_norm"]
    assert math.isfinite(gn) and gn > 0, steps[-1]


class _Odd(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n)) for n in sizes])


def _check_table(flat, ranges):
    from ddpx.ops.clip import CHUNK, GradNormPlan
    plan = GradNormPlan(flat, ranges)
    cover = torch.zeros(flat.total, dtype=torch.int32)
    is_param = torch.zeros(flat.total, dtype=torch.bool)
    owner = torch.full((flat.total,), -1, dtype=torch.int64)
    for i, (o, n) in enumerate(zip(flat.offsets, flat.numels)):
        is_param[o:o + n] = True
        owner[o:o + n] = i
    in_range = torch.zeros(flat.total, dtype=torch.bool)
    for s, e in ranges:
        in_range[s:e] = True
    assert plan.table.shape == (plan.n_chunks, 2) and plan.table.dtype == torch.int64
    for s, n in plan.table.tolist():
        assert 1 <= n <= CHUNK
        assert (s * 2) % 16 == 0 and (s * 4) % 16 == 0  # 16-B aligned as bf16 and as fp32
        assert len(set(owner[s:s + n].tolist())) == 1 and owner[s] >= 0  # inside ONE parameter, no padding
        cover[s:s + n] += 1
    want = (is_param & in_range).to(torch.int32)
    assert torch.equal(cover, want)  # every parameter element of the ranges exactly once, padding never
    assert sum(c for _, c in plan.spans) == plan.n_chunks
    return plan


def test_chunk_table_covers_parameters_once_before_and_after_relayout():
    from ddpx.ops.clip import CHUNK, GradNormPlan
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(0)
    sizes = [1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 5, 2 * CHUNK + 1]
    flat = FlatParams(_Odd(sizes))
    plan = _check_table(flat, [(0, flat.total)])
    # a shard boundary in the middle of the biggest parameter, 64-element aligned
    big = flat.numels.index(2 * CHUNK + 1)
    cut = flat.offsets[big] + 64 * 300
    _check_table(flat, [(0, cut)])
    _check_table(flat, [(cut, flat.total)])
    _check_table(flat, [(0, cut), (cut, flat.total)])
    v0 = flat.layout_version
    n = len(flat.params)
    flat.relayout([list(range(0, n, 2)), list(range(1, n, 2))], pad_to=256)
    assert flat.layout_version == v0 + 1
    _check_table(flat, [(0, flat.total)])
    for s, e in flat.group_spans:
        half = s + (e - s) // 2
        assert half % 64 == 0
        _check_table(flat, [(s, half)])
        _check_table(flat, [(half, e)])
    # a plan made before a relayout rebuilds its table for the new layout, once
    plan = GradNormPlan(flat)
    old = plan.table
    flat.relayout([list(range(n))], pad_to=256)
    flat.grad.normal_()
    plan.compute(1.0)
    assert plan.table is not old
    table = plan.table
    want = math.sqrt(sum(p.main_grad.double().square().sum().item() for p in flat.params))
    assert abs(plan.norm_dev.item() - want) <= 1e-6 * want
    plan.compute(1.0)
    assert plan.table is table
    # a misaligned range boundary inside a parameter is refused, not read misaligned
    with pytest.raises(ValueError):
        _check_table(flat, [(flat.offsets[flat.numels.index(CHUNK)] + 3, flat.total)])


def test_cpu_norm_ignores_padding_and_clip_matches_torch():
    from ddpx.optim import clip_grad_norm_
    from ddpx.optim.sgd import SGD
    from ddpx.runtime.flat_params import FlatParams
    torch.manual_seed(1)
    sizes = [1, 3, 65, 700]
    for max_norm in (0.5, 1e9):
        m = _Odd(sizes)
        twin = _Odd(sizes)
        twin.load_state_dict(m.state_dict())
        flat = FlatParams(m)
        opt = SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
        topt = torch.optim.SGD(twin.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4)
        for _ in range(3):
            flat.grad.fill_(float("nan"))  # the padding stays NaN: it must never be read
            for p, q in zip(m.parameters(), twin.parameters()):
                g = torch.randn(p.shape)
                p.main_grad.copy_(g)
                flat.grad_done(p)
                q.grad = g.clone()
            opt.step()
            tn = torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
            topt.step()
            opt.zero_grad()
            assert abs(opt.grad_norm_dev.item() - tn.item()) <= 1e-6 * tn.item()
            assert opt.clip_coef_dev.item() == (1.0 if max_norm > 1 else pytest.approx(max_norm / (tn.item() + 1e-6), rel=1e-5))
        for p, q in zip(m.parameters(), twin.parameters()):
            assert torch.allclose(p, q, atol=1e-6, rtol=1e-5)
    # functional form: scales in place, returns the pre-clip norm
    m = _Odd(sizes)
    flat = FlatParams(m)
    flat.grad.fill_(float("nan"))
    gs = []
    for p in m.parameters():
        g = torch.randn(p.shape)
        p.main_grad.copy_(g)
        flat.grad_done(p)
        gs.append(g)
    want = math.sqrt(sum(g.double().square().sum().item() for g in gs))
    norm = clip_grad_norm_(m, 0.25)
    assert abs(norm.item() - want) <= 1e-6 * want
    for p, g in zip(m.parameters(), gs):
        assert torch.allclose(p.main_grad, g * (0.25 / (want + 1e-6)), rtol=1e-5, atol=0)


def test_max_grad_norm_stays_out_of_state_dict_and_turns_fused_off():
    from ddpx.optim.sgd import SGD
    from ddpx.runtime.flat_params import FlatParams
    a, b = _Odd([5, 70]), _Odd([5, 70])
    FlatParams(a)
    FlatParams(b)
    plain = SGD(a.parameters(), lr=0.1, momentum=0.9)
    clip = SGD(b.parameters(), lr=0.1, momentum=0.9, fused_backward=True, max_grad_norm=1.0)
    assert clip.state_dict()["param_groups"][0].keys() == plain.state_dict()["param_groups"][0].keys()
    assert clip.fused_active() is False and clip.max_grad_norm == 1.0
    assert plain.grad_norm_dev is None and plain.max_grad_norm is None
    with pytest.raises(ValueError):
        SGD(_prep([4]).parameters(), lr=0.1, max_grad_norm=0.0)


def _prep(sizes):
    from ddpx.runtime.flat_params import FlatParams
    m = _Odd(sizes)
    FlatParams(m)
    return m
