"""Sharded evaluation with two ranks sharing ONE MI355X (``HostStagedComm``), in the shape of
``tests/test_gpu_ema_multirank.py``: MLP, synthetic test set of 1003, batch 128.

Each rank evaluates its half (rank 1's last batch carries one padded row) and the sums are added over gloo: the
counts equal rank 0's unsharded ones exactly, the loss to 1e-12 relative (fp64 partial sums in another order), and
both ranks hold the same numbers.  Under ZeRO-1 with deferred all-gathers, the Trainer's validation right after a
step reads fully gathered weights: it equals an evaluation after an explicit ``consolidate()``.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_gloo

pytestmark = pytest.mark.gpu


def _worker(rank, ws, port, tmp, errq):
    import torch.distributed as dist
    try:
        import ddpx
        from ddpx.data.datasets import synthetic_cifar
        from ddpx.data.loader import DeviceLoader
        from ddpx.data.sampler import DistributedIndexSampler
        from ddpx.models import MLP
        from ddpx.optim.sgd import SGD
        from ddpx.parallel.comm import HostStagedComm
        from ddpx.parallel.ddp import DistributedDataParallel
        from ddpx.train.evaluate import evaluate_metrics
        from ddpx.train.trainer import Trainer
        init_gloo(rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        torch.manual_seed(7 + rank)  # different init per rank: the wrap brings rank 0's weights
        ours = MLP(hidden=512)
        ddpx.prepare_model(ours, dev)
        d = DistributedDataParallel(ours, comm=HostStagedComm(), bucket_cap_mb=1.0, first_bucket_mb=0.25,
                                    overlap_optimizer=True, shard_optimizer=True, defer_gather=True)
        assert d.sharded and d.defer_gather
        o = SGD(ours.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        d.attach_optimizer(o)

        test_set = synthetic_cifar(1003, seed=5)
        whole_data = DeviceLoader(test_set, 128, dev, train=False, layout="flat_bf16")
        part_data = DeviceLoader(test_set, 128, dev, train=False, layout="flat_bf16",
                                 sampler=DistributedIndexSampler(len(test_set), ws, rank, shuffle=False))
        assert sum(part_data.valid_rows(s) for s in range(len(part_data))) == (502 if rank == 0 else 501)

        def same(a, b):
            assert (a.top1, a.topk, a.k, a.samples) == (b.top1, b.topk, b.k, b.samples), (rank, a, b)  # counts: exact
            assert abs(a.loss - b.loss) <= 1e-12 * abs(b.loss), (rank, a.loss, b.loss)

        def on_both(res):
            got = [None] * ws
            dist.all_gather_object(got, tuple(res))
            assert all(g == got[0] for g in got), got
            return got

        # 1. sharded against unsharded
        whole = evaluate_metrics(ours, whole_data, topk=5, progress=False)
        part = evaluate_metrics(ours, part_data, topk=5, comm_group=dist.group.WORLD, progress=False)
        assert whole.samples == 1003 and whole.loss == whole.loss
        same(part, whole)
        on_both(part)      # both ranks report identical numbers
        on_both(whole)     # (and rank 0's unsharded ones are every rank's)

        # 2. ZeRO-1, deferred all-gathers: the validation that follows the epoch's last step
        train = DeviceLoader(synthetic_cifar(256, seed=4), 64, dev, train=True, layout="flat_bf16", seed=2,
                             sampler=DistributedIndexSampler(256, ws, rank, shuffle=True))
        sched = torch.optim.lr_scheduler.LambdaLR(o, lambda s: 1.0 / (1 + s))
        tr = Trainer(d, train, o, 0, 10 ** 9, sched, distributed=True, rank=rank, ckpt_path=f"{tmp}/checkpoint.pt",
                     val_data=part_data, eval_every=1, topk=5)
        pending = []
        inner = tr._validate

        def spy(epoch):
            pending.append(len(d._gather_todo))
            return inner(epoch)
        tr._validate = spy
        tr.train(1)
        assert pending and pending[0] > 0, "the step left all-gathers deferred: the validation has to issue them"
        after_step = tr.last_eval
        d.consolidate()
        torch.cuda.synchronize()
        settled = evaluate_metrics(ours, part_data, topk=5, comm_group=dist.group.WORLD, progress=False)
        same(after_step, settled)
        assert (after_step.loss, after_step.top1) != (whole.loss, whole.top1), "training moved the model"
        on_both(after_step)
        same(evaluate_metrics(ours, whole_data, topk=5, progress=False), settled)
        d.close()
        dist.destroy_process_group()
    except BaseException as e:  # report through the queue: spawn's own traceback loses assertion text
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_sharded_evaluation_two_ranks_one_gpu(gpu, tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_worker, args=(2, free_port(), str(tmp_path), q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")
