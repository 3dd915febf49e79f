"""Gradient clipping with two ranks sharing ONE MI355X (``HostStagedComm``): replicated DDP with optimizer
overlap and ZeRO-1, each with ``SGD(max_grad_norm=...)``.

As in ``tests/test_gpu_multirank.py`` every rank checks its result against a single-process ddpx model that runs
the per-rank half batches of the concatenated batch one after the other and accumulates ``loss_r / ws`` (with
ws = 2 the scale is exact, so the activations round exactly as on the ranks), here with the same clipping
optimizer; the tolerances are that file's.  The pre-clip norm must be the same bits on both ranks in both modes,
and the ZeRO-1 norm (shard partial sums + one scalar all-reduce) must equal the replicated one within the
summation bound of ``tests/test_gpu_clip.py``: at the first step both modes hold bit-identical reduced gradients
(the host-staged fp32 sum of the two ranks), so only the split of the sum differs.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo
from tests.test_gpu_clip import BOUND

pytestmark = pytest.mark.gpu

MAX_NORM = 0.05


def _worker(rank, ws, port, grad_dtype, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.models import MLP
        from ddpx.optim.sgd import SGD
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        gd = torch.bfloat16 if grad_dtype == "bf16" else torch.float32
        norms = {}
        for shard in (False, True):
            torch.manual_seed(7 + rank)  # different init per rank: DDP must broadcast rank 0's weights
            ours = MLP(hidden=512)
            torch.manual_seed(7)
            ref = MLP(hidden=512)  # rank 0's init
            ddpx.prepare_model(ours, dev, grad_dtype=gd)
            ddpx.prepare_model(ref, dev)
            d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                        overlap_optimizer=True, shard_optimizer=shard)
            assert d.sharded == shard
            o = SGD(ours.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=MAX_NORM)
            d.attach_optimizer(o)
            o_ref = SGD(ref.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=MAX_NORM)
            w0 = [p.detach().clone() for p in ref.parameters()]
            B = 128
            norms[shard] = []
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
                n_mine = o.grad_norm_dev.detach().cpu().reshape(1)
                both = [torch.empty(1) for _ in range(ws)]
                dist.all_gather(both, n_mine)
                assert all(torch.equal(v, both[0]) for v in both), ("norm differs across ranks", shard, s, both)
                n_ref = o_ref.grad_norm_dev.item()
                assert n_ref > MAX_NORM, "the clip must be active"
                assert abs(n_mine.item() - n_ref) < (2e-2 if grad_dtype == "bf16" else 5e-4) * n_ref, (shard, s)
                norms[shard].append(n_mine.item())
            d.consolidate()
            torch.cuda.synchronize()
            for (n, p), q, p0 in zip(ours.named_parameters(), ref.parameters(), w0):
                du, dr = (p - p0).double(), (q - p0).double()
                rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                tol = 2e-2 if grad_dtype == "bf16" else 5e-4  # tests/test_gpu_multirank.py
                assert rel < tol, (rank, shard, n, rel)
            so, sr = o.state_dict()["state"], o_ref.state_dict()["state"]
            for i in sr:
                a, b = so[i]["momentum_buffer"].double(), sr[i]["momentum_buffer"].double()
                rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
                assert rel < (5e-2 if grad_dtype == "bf16" else 5e-4), (shard, i, rel)
            flat = ours.fc0.weight._ddpx_flat.master.detach().cpu()
            lst = [torch.empty_like(flat) for _ in range(ws)]
            dist.all_gather(lst, flat)
            for other in lst:
                assert torch.equal(other, lst[0]), "replicas diverged"
            d.close()
        a, b = norms[False][0], norms[True][0]
        print(f"rank {rank} first-step norm: replicated {a!r} ZeRO-1 {b!r}", flush=True)
        assert abs(a - b) <= BOUND * a, (a, b)
        dist.destroy_process_group()
    except BaseException as e:  # report through the queue: spawn's own traceback loses assertion text
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


@pytest.mark.parametrize("grad_dtype", ["fp32", "bf16"])
def test_clip_two_ranks_one_gpu(gpu, grad_dtype):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), grad_dtype, 3, q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
