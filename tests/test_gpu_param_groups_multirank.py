"""Two-group SGD and AdamW (``ddpx.optim.decay_groups``: no weight decay on the biases) with two ranks sharing ONE
MI355X (``HostStagedComm``): replicated DDP with optimizer overlap (one table-driven launch per bucket as its
all-reduce lands), and ZeRO-1 (shards that cut a weight matrix in two; the hyper table is rebuilt for the re-laid-out
store and is the same on every rank).

As in ``tests/test_gpu_adamw_multirank.py`` every rank checks its result against a single-process ddpx model with the
same groups that runs the per-rank half batches of the concatenated batch one after the other and accumulates
``loss_r / ws``; the tolerances are that file's (fp32 gradient buffers, for the reason given there).  After 3 steps
every rank holds the same weights.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu

KINDS = {"sgd": (dict(lr=0.1, momentum=0.9), 5e-4, ("momentum_buffer",)),
         "adamw": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), 0.01, ("exp_avg", "exp_avg_sq"))}


def _worker(rank, ws, port, kind, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        import ddpx.optim
        from ddpx.models import MLP
        from ddpx.optim import decay_groups
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        hp, wd, state_keys = KINDS[kind]
        cls = ddpx.optim.SGD if kind == "sgd" else ddpx.optim.AdamW
        for shard in (False, True):
            torch.manual_seed(7 + rank)  # different init per rank: DDP must broadcast rank 0's weights
            ours = MLP(hidden=512)
            torch.manual_seed(7)
            ref = MLP(hidden=512)  # rank 0's init
            ddpx.prepare_model(ours, dev)
            ddpx.prepare_model(ref, dev)
            # the optimizer first, as the training scripts build it: its state follows the sharded re-layout
            o = cls(decay_groups(ours, wd), allow_groups=True, **hp)
            d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                        overlap_optimizer=True, shard_optimizer=shard)
            assert d.sharded == shard
            d.attach_optimizer(o)
            o_ref = cls(decay_groups(ref, wd), allow_groups=True, **hp)
            for opt in (o, o_ref):
                h = opt._hyper()
                assert len(opt.param_groups) == 2 and not h.uniform and not opt.fused_active()
                assert h.table is not None and sorted(set(h.wd)) == [0.0, wd] and set(h.lr_mul) == {1.0}
                f = opt.flat
                assert all((h.wd[f.index[id(p)]] == 0.0) == (p.dim() <= 1) for p in f.params)
            if shard:
                f, split = o.flat, False
                for b in range(len(d.bucket_ranges)):
                    if d.bucket_modes[b] == 1:
                        cut = d.bucket_ranges[b][0] + (d.bucket_ranges[b][1] - d.bucket_ranges[b][0]) // ws
                        split |= any(off < cut < off + n and p.dim() > 1
                                     for off, n, p in zip(f.offsets, f.numels, f.params))
                assert split, "a shard boundary must fall inside a weight matrix"
            w0 = [p.detach().clone() for p in ref.parameters()]
            B = 128
            for s in range(steps):
                g = torch.Generator(device="cpu").manual_seed(1000 + s)
                xg = torch.rand(ws * B, 3072, generator=g).to(dev).to(torch.bfloat16)
                tg = torch.randint(0, 10, (ws * B,), generator=g).to(dev)
                o.zero_grad()
                loss, _ = d.forward_loss(xg[rank * B:(rank + 1) * B], tg[rank * B:(rank + 1) * B])
                loss.backward()
                o.step()
                o_ref.zero_grad()
                for r in range(ws):
                    lr_, _ = ref.forward_loss(xg[r * B:(r + 1) * B], tg[r * B:(r + 1) * B])
                    (lr_ / ws).backward()
                o_ref.step()
            torch.cuda.synchronize()
            assert o.step_count == steps
            d.consolidate()
            torch.cuda.synchronize()
            tol = 5e-4  # tests/test_gpu_multirank.py, fp32 gradients
            for (n, p), q, p0 in zip(ours.named_parameters(), ref.parameters(), w0):
                du, dr = (p - p0).double(), (q - p0).double()
                rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                assert rel < tol, (rank, shard, n, rel)
            so, sr = o.state_dict(), o_ref.state_dict()
            assert [g["params"] for g in so["param_groups"]] == [g["params"] for g in sr["param_groups"]]
            for i in sr["state"]:
                for k in state_keys:
                    a, b = so["state"][i][k].double(), sr["state"][i][k].double()
                    rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
                    assert rel < 5e-4, (shard, i, k, rel)
            flat = ours.fc0.weight._ddpx_flat.master.detach().cpu()
            lst = [torch.empty_like(flat) for _ in range(ws)]
            dist.all_gather(lst, flat)
            for other in lst:
                assert torch.equal(other, lst[0]), "replicas diverged"
            d.close()
        dist.destroy_process_group()
    except BaseException as e:  # report through the queue: spawn's own traceback loses assertion text
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_two_groups_two_ranks_one_gpu(gpu, kind):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), kind, 3, q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
