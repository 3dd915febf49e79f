"""``ddpx.optim.LARS`` with two ranks sharing ONE MI355X (``HostStagedComm``): replicated DDP with optimizer
overlap, and ZeRO-1, with fp32 and bf16 gradient buffers.

As in ``tests/test_gpu_adamw_multirank.py`` every rank checks its result against a single-process ddpx model that
runs the per-rank half batches of the concatenated batch one after the other and accumulates ``loss_r / ws``; the
tolerances are that file's (``tests/test_gpu_multirank.py``'s: 5e-4 on the update, relative by norm, with fp32
gradient buffers, 2e-2 with bf16 ones; 5e-2 on the state with bf16 ones).  LARS' update is SGD's times one scalar per
parameter, so its error is proportional to the gradient's, as those tolerances presume; the scalar itself moves with
the gradient norm, by no more than the gradient's own relative error.

Those tolerances are for a step taken from the SAME weights and momentum, so the single process takes over the
ranks' (consolidated) state before every step and each of the 3 steps is compared, as
``tests/test_gpu_clip.py::test_native_mlp_clipped_steps_match_torch_twin`` does and for the reason written there:
with bf16 gradient buffers the rounding of step 1's gradient moves the weights enough to flip bf16 roundings and
ReLU decisions of later activations, and a reference left on its own trajectory then measures that divergence, which
grows with the step size, not the kernels.  Measured with these hyper-parameters (0.8 % of a weight matrix's norm
per step) on free trajectories: fc0.weight's 3-step update 2.6e-2 apart with bf16 buffers while every fp32-buffer
comparison stayed inside 5e-4.

The trust table must be the same bits on both ranks in both modes: the replicated plan reduces identical gradients
with identical tables; under ZeRO-1 each rank sums w^2 and g^2 over its own pieces of master and gradient and one
all-reduce of the [2 P] vector completes the totals (a weight matrix is split across the two shards).
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu

HP = dict(lr=0.4, momentum=0.9, weight_decay=5e-4, trust_coef=0.02, eps=1e-8, max_grad_norm=0.05)


def _worker(rank, ws, port, grad_dtype, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.models import MLP
        from ddpx.optim import LARS
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
            o = LARS(ours.parameters(), **HP)
            d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                        overlap_optimizer=True, shard_optimizer=shard)
            assert d.sharded == shard
            d.attach_optimizer(o)
            f = o.flat
            if shard:
                split = False
                for b in range(len(d.bucket_ranges)):
                    if d.bucket_modes[b] == 1:
                        s0, e0 = d.bucket_ranges[b]
                        cut = s0 + (e0 - s0) // ws
                        split |= any(off < cut < off + n for off, n in zip(f.offsets, f.numels))
                assert split, "a parameter must be split across the two shards"
            o_ref = LARS(ref.parameters(), **HP)
            f_ref = o_ref.flat
            B = 128
            tol = 2e-2 if grad_dtype == "bf16" else 5e-4  # tests/test_gpu_multirank.py
            mtol = 5e-2 if grad_dtype == "bf16" else 5e-4
            pairs = list(zip(ours.named_parameters(), ref.parameters()))
            for s in range(steps):
                # the single process takes over the ranks' state (complete on every rank after consolidate)
                d.consolidate()
                with torch.no_grad():
                    for (_, p), q in pairs:
                        q.copy_(p)
                        o_ref.momentum_buffer[f_ref.slice(f_ref.index[id(q)])].copy_(
                            o.momentum_buffer[f.slice(f.index[id(p)])])
                    f_ref.refresh_shadow()
                w0 = [q.detach().clone() for q in ref.parameters()]
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
                mine = o.trust_ratio_dev.detach().cpu()
                lst = [torch.empty_like(mine) for _ in range(ws)]
                dist.all_gather(lst, mine)
                assert all(torch.equal(t, lst[0]) for t in lst), ("trust tables differ across ranks", shard, s, lst)
                norms = [torch.empty(1) for _ in range(ws)]
                dist.all_gather(norms, o.grad_norm_dev.detach().cpu().reshape(1))
                assert all(torch.equal(t, norms[0]) for t in norms), (shard, s, norms)
                for (n, p), q in pairs:
                    a = mine[f.index[id(p)]].item()
                    b = o_ref.trust_ratio_dev[f_ref.index[id(q)]].item()
                    assert (a == 1.0) == (p.dim() <= 1) and abs(a - b) <= tol * b, (rank, shard, s, n, a, b)
                assert o_ref.clip_coef_dev.item() < 1.0, "the clip must be active"
                d.consolidate()
                torch.cuda.synchronize()
                for ((n, p), q), p0 in zip(pairs, w0):
                    du, dr = (p - p0).double(), (q - p0).double()
                    rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                    assert rel < tol, (rank, shard, s, n, rel)
                    a = o.momentum_buffer[f.slice(f.index[id(p)])].double()
                    b = o_ref.momentum_buffer[f_ref.slice(f_ref.index[id(q)])].double()
                    rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
                    assert rel < mtol, (rank, shard, s, n, "momentum", rel)
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


@pytest.mark.parametrize("grad_dtype", ["fp32", "bf16"])
def test_lars_two_ranks_one_gpu(gpu, grad_dtype):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), grad_dtype, 3, q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
