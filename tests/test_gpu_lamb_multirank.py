"""``ddpx.optim.LAMB`` with two ranks sharing ONE MI355X (``HostStagedComm``): replicated DDP with optimizer
overlap, and ZeRO-1, with fp32 and bf16 gradient buffers, and one clipped ZeRO-1 case.

As in ``tests/test_gpu_lars_multirank.py`` every rank checks its result against a single-process ddpx model that
runs the per-rank half batches of the concatenated batch one after the other and accumulates ``loss_r / ws``; the
tolerances are that file's (``tests/test_gpu_multirank.py``'s: 5e-4 on the update, relative by norm, with fp32
gradient buffers, 2e-2 with bf16 ones; 5e-2 on the state with bf16 ones), and, as there and for the reason written
there, they are for a step taken from the SAME weights and state: the single process takes over the ranks'
(consolidated) weights, exp_avg and exp_avg_sq before every step and each of the 3 steps is compared.  Both sides
count their steps alike, so the bias corrections agree.

Those tolerances presume an update whose error is proportional to the gradient's, and ``eps`` decides whether
LAMB's is.  The direction r = m^ / (sqrt(v^) + eps) is sign(g)-like wherever |g| >> eps (+-1 at step 1), and
``tests/test_gpu_adamw_multirank.py`` says what follows with bf16 gradient buffers: where the two ranks'
contributions nearly cancel, rounding each to bf16 (relative 2^-9) before the sum flips the sign of the summed
gradient; about 4e-4 to 1e-3 of the elements move by 2 |r| instead of 0, a relative update error of 2e-2 to 4e-2
whatever the kernels do (measured here with eps = 1e-6: fc2.weight's step-1 update 2.5e-2 apart on both ranks, every
other parameter inside 2e-2).  That file therefore runs fp32 buffers only.  Here the bf16 case stays, at the same
tolerance, with ``eps`` = 1e-3 (``EPS``), chosen from the number formats and the model, not from a result:
an element's direction then moves by at most d / eps for a gradient error d <= 2 * 2^-9 G (G: the size of a rank's
contribution), so a flipped element moves by at most 4e-3 G / eps instead of 2, and G <= 0.1 for every layer of this
model at these inputs (|dL/dlogit| <= 1 / element, activations of order 1, batch mean): at most 0.4 on 1e-3 of
the elements, 1.3e-2 of the update by norm in the worst layer, and the gradient's own 2^-9 elsewhere.  With fp32
buffers the flip needs a cancellation to 2^-24 and the cases run at LAMB's default eps = 1e-6.  The trust ratio
moves with the update's norm, by no more than the update's relative error.

The trust table must be the same bits on both ranks in both modes: the replicated plan reduces identical gradients
with identical tables; under ZeRO-1 each rank sums w^2 and u^2 over its own pieces of master and state and one
all-reduce of the [2 P] vector completes the totals (a weight matrix is split across the two shards).
"""
import time

import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=0.01)
EPS = {"fp32": 1e-6, "bf16": 1e-3}  # (the module docstring)
LIMIT = 240.0  # seconds for the two children of one case


def _worker(rank, ws, port, grad_dtype, modes, max_norm, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.models import MLP
        from ddpx.optim import LAMB
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        gd = torch.bfloat16 if grad_dtype == "bf16" else torch.float32
        hp = dict(HP, eps=EPS[grad_dtype], max_grad_norm=max_norm)
        for shard in modes:
            torch.manual_seed(7 + rank)  # different init per rank: DDP must broadcast rank 0's weights
            ours = MLP(hidden=512)
            torch.manual_seed(7)
            ref = MLP(hidden=512)  # rank 0's init
            ddpx.prepare_model(ours, dev, grad_dtype=gd)
            ddpx.prepare_model(ref, dev)
            # the optimizer first, as the training scripts build it: its state follows the sharded re-layout
            o = LAMB(ours.parameters(), **hp)
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
            else:
                assert len(d.bucket_ranges) >= 2
            o_ref = LAMB(ref.parameters(), **hp)
            f_ref = o_ref.flat
            B = 128
            tol = 2e-2 if grad_dtype == "bf16" else 5e-4  # tests/test_gpu_multirank.py
            mtol = 5e-2 if grad_dtype == "bf16" else 5e-4
            pairs = list(zip(ours.named_parameters(), ref.parameters()))
            worst = [0.0, 0.0, 0.0]
            for s in range(steps):
                # the single process takes over the ranks' state (complete on every rank after consolidate)
                d.consolidate()
                with torch.no_grad():
                    for (_, p), q in pairs:
                        q.copy_(p)
                        sl, slr = f.slice(f.index[id(p)]), f_ref.slice(f_ref.index[id(q)])
                        o_ref.exp_avg[slr].copy_(o.exp_avg[sl])
                        o_ref.exp_avg_sq[slr].copy_(o.exp_avg_sq[sl])
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
                assert o.steps_taken() == s + 1 and o_ref.steps_taken() == s + 1
                mine = o.trust_ratio_dev.detach().cpu()
                lst = [torch.empty_like(mine) for _ in range(ws)]
                dist.all_gather(lst, mine)
                assert all(torch.equal(t, lst[0]) for t in lst), ("trust tables differ across ranks", shard, s, lst)
                if max_norm is not None:
                    norms = [torch.empty(1) for _ in range(ws)]
                    dist.all_gather(norms, o.grad_norm_dev.detach().cpu().reshape(1))
                    assert all(torch.equal(t, norms[0]) for t in norms), (shard, s, norms)
                    assert o_ref.clip_coef_dev.item() < 1.0, "the clip must be active"
                for (n, p), q in pairs:
                    a = mine[f.index[id(p)]].item()
                    b = o_ref.trust_ratio_dev[f_ref.index[id(q)]].item()
                    assert (a == 1.0) == (p.dim() <= 1) and abs(a - b) <= tol * b, (rank, shard, s, n, a, b)
                    worst[0] = max(worst[0], abs(a - b) / (tol * b))
                d.consolidate()
                torch.cuda.synchronize()
                for ((n, p), q), p0 in zip(pairs, w0):
                    du, dr = (p - p0).double(), (q - p0).double()
                    rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                    assert rel < tol, (rank, shard, s, n, rel)
                    worst[1] = max(worst[1], rel / tol)
                    sl, slr = f.slice(f.index[id(p)]), f_ref.slice(f_ref.index[id(q)])
                    for name, x, y in (("exp_avg", o.exp_avg, o_ref.exp_avg),
                                       ("exp_avg_sq", o.exp_avg_sq, o_ref.exp_avg_sq)):
                        a, b = x[sl].double(), y[slr].double()
                        rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
                        assert rel < mtol, (rank, shard, s, n, name, rel)
                        worst[2] = max(worst[2], rel / mtol)
            if rank == 0:
                print(f"lamb 2 ranks {grad_dtype} shard {shard} max_norm {max_norm}: achieved fraction of the "
                      f"tolerance: trust {worst[0]:.3f} update {worst[1]:.3f} state {worst[2]:.3f}", flush=True)
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


@pytest.mark.parametrize("grad_dtype,modes,max_norm", [("fp32", (False, True), None), ("bf16", (False, True), None),
                                                       ("fp32", (True,), 0.05)],
                         ids=["g32", "g16", "g32-zero1-clip"])
def test_lamb_two_ranks_one_gpu(gpu, grad_dtype, modes, max_norm):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    pc = mp.spawn(_worker, args=(2, free_port(), grad_dtype, modes, max_norm, 3, q), nprocs=2, join=False)
    deadline = time.monotonic() + LIMIT
    try:
        while not pc.join(timeout=2.0):  # (raises when a child failed)
            if time.monotonic() > deadline:
                raise TimeoutError(f"the two ranks did not finish within {LIMIT:.0f} s")
    except Exception as e:
        for p in pc.processes:
            if p.is_alive():
                p.kill()
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or f"worker failed: {e!r}")
