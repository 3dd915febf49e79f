"""``ddpx.optim.AdamW`` with two ranks sharing ONE MI355X (``HostStagedComm``): replicated DDP with optimizer
overlap, and ZeRO-1.

As in ``tests/test_gpu_clip_multirank.py`` every rank checks its result against a single-process ddpx model that
runs the per-rank half batches of the concatenated batch one after the other and accumulates ``loss_r / ws``; the
tolerances are that file's.  After 3 steps every rank holds the same weights; under ZeRO-1, before consolidation,
a rank's ``exp_avg`` / ``exp_avg_sq`` are non-zero only where it updates: its shard of every sharded bucket and
the replicated buckets.

fp32 gradient buffers only, for a reason in the number formats: the reference accumulates fp32 gradients, and that
file's tolerances (5e-4 on the update, relative, by norm) presume an update whose error is proportional to the
gradient's, as SGD's is.  AdamW's first updates are lr * sign(g)-like (m^ / sqrt(v^) = +-1 at step 1): where the
two ranks' contributions nearly cancel, rounding each to bf16 (relative 2^-9) before the sum can flip the sign of
the summed gradient, and such an element moves by 2 lr instead of 0.  With two equally noisy halves that is about
4e-4 of the elements, a relative update error of about sqrt(4e-4) * 2 = 4e-2 whatever the kernel does: no check
of it.  In fp32 the same flip needs a cancellation to 2^-24 (about 1e-7 of the elements: an error of 6e-4 of one
element's update, far below the tolerance).  bf16 gradients through the kernel are covered element by element
in ``tests/test_gpu_adamw.py``.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _worker(rank, ws, port, grad_dtype, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.models import MLP
        from ddpx.optim import AdamW
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        gd = torch.bfloat16 if grad_dtype == "bf16" else torch.float32
        for shard in (False, True):
            torch.manual_seed(7 + rank)  # different init per rank: DDP must broadcast rank 0's weights
            ours = MLP(hidden=512)
            torch.manual_seed(7)
            ref = MLP(hidden=512)  # rank 0's init
            ddpx.prepare_model(ours, dev, grad_dtype=gd)
            ddpx.prepare_model(ref, dev)
            # the optimizer first, as the training scripts build it: its state follows the sharded re-layout
            o = AdamW(ours.parameters(), **HP)
            d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                        overlap_optimizer=True, shard_optimizer=shard)
            assert d.sharded == shard
            d.attach_optimizer(o)
            o_ref = AdamW(ref.parameters(), **HP)
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
            assert o.step_dev.item() == steps
            if shard:
                mine = torch.zeros(o.flat.total, dtype=torch.bool, device=dev)
                nsh = 0
                for b in range(len(d.bucket_ranges)):
                    nsh += int(d.bucket_modes[b] == 1)
                    for (s0, e0) in d.update_ranges(b):
                        mine[s0:e0] = True
                assert nsh > 0 and not mine.all(), "the plan must shard something"
                for name in ("exp_avg", "exp_avg_sq"):
                    t = o.flat.state_tensors[name]
                    assert (t[~mine] == 0).all(), (rank, name, "state outside this rank's ranges")
                    assert t[mine].abs().sum().item() > 0, (rank, name)
            d.consolidate()
            torch.cuda.synchronize()
            tol = 2e-2 if grad_dtype == "bf16" else 5e-4  # tests/test_gpu_multirank.py
            for (n, p), q, p0 in zip(ours.named_parameters(), ref.parameters(), w0):
                du, dr = (p - p0).double(), (q - p0).double()
                rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                assert rel < tol, (rank, shard, n, rel)
            so, sr = o.state_dict()["state"], o_ref.state_dict()["state"]
            for i in sr:
                for k in ("exp_avg", "exp_avg_sq"):
                    a, b = so[i][k].double(), sr[i][k].double()
                    rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
                    assert rel < (5e-2 if grad_dtype == "bf16" else 5e-4), (shard, i, k, rel)
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


@pytest.mark.parametrize("grad_dtype", ["fp32"])
def test_adamw_two_ranks_one_gpu(gpu, grad_dtype):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), grad_dtype, 3, q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
