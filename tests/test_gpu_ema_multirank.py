"""``ddpx.optim.WeightEMA`` with two ranks sharing ONE MI355X (``HostStagedComm``): replicated DDP with optimizer
overlap, and ZeRO-1.

The pattern and the tolerance are ``tests/test_gpu_adamw_multirank.py``'s (fp32 gradient buffers, 3 AdamW steps,
5e-4 relative, by norm, per parameter): every rank checks its average against that of a single-process ddpx model
that runs the per-rank half batches one after the other.  The average is attached before the model is wrapped, as
the training scripts do it, and every rank initialises its model differently: the wrap must leave rank 0's weights
in every rank's average.  Under ZeRO-1, before consolidation, a rank's average has moved only where the rank
updates (its shard of every sharded bucket and the replicated buckets) and is rank 0's initial weights elsewhere;
``consolidate()`` completes it.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
DECAY = 0.9
TOL = 5e-4  # tests/test_gpu_adamw_multirank.py, fp32 gradients


def _worker(rank, ws, port, steps, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.models import MLP
        from ddpx.optim import AdamW, WeightEMA
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        for shard in (False, True):
            torch.manual_seed(7 + rank)  # different init per rank: the wrap must bring rank 0's weights AND average
            ours = MLP(hidden=512)
            torch.manual_seed(7)
            ref = MLP(hidden=512)  # rank 0's init
            ddpx.prepare_model(ours, dev)
            ddpx.prepare_model(ref, dev)
            o = AdamW(ours.parameters(), **HP)
            ema = WeightEMA(o, decay=DECAY)
            d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                        overlap_optimizer=True, shard_optimizer=shard)
            assert d.sharded == shard
            d.attach_optimizer(o)
            o_ref = AdamW(ref.parameters(), **HP)
            ema_ref = WeightEMA(o_ref, decay=DECAY)
            w0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
            f = o.flat

            def avg_of(e, opt, model):
                fl = opt.flat
                return {n: e.buffer[fl.slice(fl.index[id(p)])].view(p.shape) for n, p in model.named_parameters()}

            init = f.master.clone()  # (in the layout the wrap left)
            assert torch.equal(ema.buffer, init), (rank, "the average must start as the broadcast weights")
            for n, a in avg_of(ema, o, ours).items():
                assert torch.equal(a, w0[n]), (rank, n, "not rank 0's initial weights")
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
            assert ema.counts() == (steps, steps) == ema_ref.counts()
            if shard:
                mine = torch.zeros(f.total, dtype=torch.bool, device=dev)
                nsh = 0
                for b in range(len(d.bucket_ranges)):
                    nsh += int(d.bucket_modes[b] == 1)
                    for (s0, e0) in d.update_ranges(b):
                        mine[s0:e0] = True
                assert nsh > 0 and not mine.all(), "the plan must shard something"
                assert torch.equal(ema.buffer[~mine], init[~mine]), (rank, "average outside this rank's ranges")
                assert not torch.equal(ema.buffer[mine], init[mine]), (rank, "average inside them did not move")
            d.consolidate()
            torch.cuda.synchronize()
            mine_avg, ref_avg = avg_of(ema, o, ours), avg_of(ema_ref, o_ref, ref)
            for n in w0:
                du, dr = (mine_avg[n] - w0[n]).double(), (ref_avg[n] - w0[n]).double()
                assert dr.norm().item() > 0
                rel = ((du - dr).norm() / dr.norm().clamp_min(1e-12)).item()
                assert rel < TOL, (rank, shard, n, rel)
            flat = ema.buffer.detach().cpu()
            lst = [torch.empty_like(flat) for _ in range(ws)]
            dist.all_gather(lst, flat)
            for other in lst:
                assert torch.equal(other, lst[0]), "the ranks' averages differ"
            # the averaged model through applied(): collective, and the training weights come back
            master, avg = f.master.clone(), ema.buffer.clone()
            with ema.applied():
                assert torch.equal(f.master, avg) and torch.equal(ema.buffer, master)
            assert torch.equal(f.master, master) and torch.equal(ema.buffer, avg)
            d.close()
        dist.destroy_process_group()
    except BaseException as e:  # report through the queue: spawn's own traceback loses assertion text
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_ema_two_ranks_one_gpu(gpu):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), 3, q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
