"""Validation on the CPU: ``eval_metrics``' torch twin against the numpy reference, ``evaluate_metrics`` against
``evaluate()``, the sharded test loader's partition, a two-process sharded evaluation over gloo, and the Trainer /
CLI ends (``--eval_every``, ``--topk``, ``--save_best``)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ddpx
from ddpx.data.datasets import synthetic_cifar
from ddpx.data.loader import DeviceLoader
from ddpx.data.sampler import DistributedIndexSampler
from ddpx.models import MLP
from ddpx.ops.head import EvalAccumulator, eval_metrics
from ddpx.optim import SGD
from ddpx.optim.schedule import one_cycle
from ddpx.runtime.flat_params import flat_of
from ddpx.train.evaluate import EvalResult, evaluate, evaluate_metrics
from ddpx.train.trainer import Trainer
from ddpx.utils.metrics import MetricsWriter
from tests._dist_util import free_port, init_gloo
from tests._eval_ref import gaussian_logits, grid_logits, ref_metrics, ties_at_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
SHAPES = [(1, 1, 1), (3, 10, 1), (17, 10, 5), (64, 16, 16), (65, 17, 5), (33, 100, 5), (16, 128, 128), (5, 130, 3)]


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(b), 1e-300)


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("M,C,k", SHAPES)
def test_cpu_twin_matches_the_numpy_reference(M, C, k, kind):
    z, t = (gaussian_logits if kind == "gaussian" else grid_logits)(M, C, seed=M * 1000 + C)
    if M > 2:
        t[1] = C + 3  # out of range: a miss, no loss
    for mv in sorted({0, 1, M // 2, M}):
        acc = EvalAccumulator(CPU)
        eval_metrics(torch.from_numpy(z), torch.from_numpy(t), acc, k, mv)
        loss, h1, hk, rows, _ = ref_metrics(z, t, k, mv)
        got = acc.read()
        assert got[1:] == (h1, hk, rows), (mv, got, (h1, hk, rows))
        assert _close(got[0], loss) or (loss == 0.0 and got[0] == 0.0), (mv, got[0], loss)


def test_cpu_twin_accumulates_and_ignores_rows_past_m_valid():
    z, t = grid_logits(32, 10, seed=5)
    assert ties_at_k(z[:19], t[:19], 3) > 0
    zp, tp = z.copy(), t.copy()
    zp[19:] = np.nan
    tp[19:] = -7
    acc = EvalAccumulator(CPU)
    for _ in range(3):
        eval_metrics(torch.from_numpy(zp), torch.from_numpy(tp), acc, 3, 19)
    loss, h1, hk, rows, _ = ref_metrics(np.concatenate([z[:19]] * 3), np.concatenate([t[:19]] * 3), 3)
    got = acc.read()
    assert got[1:] == (h1, hk, rows) and _close(got[0], loss), (got, loss, h1, hk, rows)
    with pytest.raises(ValueError):
        eval_metrics(torch.from_numpy(z), torch.from_numpy(t), acc, 11)
    with pytest.raises(ValueError):
        eval_metrics(torch.from_numpy(z), torch.from_numpy(t), acc, 1, 33)


def _mlp(seed=3, hidden=64):
    torch.manual_seed(seed)
    m = MLP(hidden=hidden)
    ddpx.prepare_model(m, CPU)
    return m


def _loader(ds, batch, model, sampler=None, train=False, seed=0):
    return DeviceLoader(ds, batch, CPU, sampler=sampler, train=train, layout=model.input_layout(CPU), seed=seed)


def test_evaluate_is_unchanged_and_equals_evaluate_metrics_top1():
    m = _mlp()
    data = _loader(synthetic_cifar(203, seed=1), 64, m)
    old = evaluate(m, data, progress=False)
    res = evaluate_metrics(m, data, progress=False)
    assert isinstance(old, float) and isinstance(res, EvalResult)
    assert res.top1 == old and res.topk is None and res.k == 1 and res.samples == 203  # the same float, bit for bit
    assert m.training
    res5 = evaluate_metrics(m, data, topk=5, progress=False)
    assert res5.top1 == old and res5.loss == res.loss and res5.k == 5 and res5.top1 <= res5.topk <= 100.0
    # against torch's own loss over the whole set
    with torch.inference_mode():
        m.eval()
        x, y = next(iter(_loader(synthetic_cifar(203, seed=1), 203, m)))
        want = torch.nn.functional.cross_entropy(m(x).double(), y).item()
        m.train()
    assert abs(res.loss - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("n", [1, 7, 10, 1003])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_shard_partition_covers_every_index_once(n, world):
    seen = []
    for rank in range(world):
        s = DistributedIndexSampler(n, world, rank, shuffle=False)
        idx = s.indices().tolist()
        valid = sum(1 for j in range(len(idx)) if rank + j * world < n)  # the reference arithmetic
        assert s.num_valid() == valid
        assert all(idx[j] == rank + j * world for j in range(valid))
        seen += idx[:valid]
        # the loader hands that prefix out batch by batch
        ds = synthetic_cifar(n, seed=2)
        ld = DeviceLoader(ds, 4, CPU, sampler=s, train=False)
        rows = [ld.valid_rows(step) for step in range(len(ld))]
        sizes = [y.numel() for _, y in ld]
        assert sum(rows) == valid and all(0 <= r <= b for r, b in zip(rows, sizes)), (rows, sizes)
        assert rows == sorted(rows, reverse=True)  # valid rows are a prefix of the rank's list
    assert sorted(seen) == list(range(n))


def _gloo_worker(rank, ws, port, errq):
    import torch.distributed as dist
    try:
        torch.set_num_threads(2)
        init_gloo(rank, ws, port)
        m = _mlp()
        ds = synthetic_cifar(1003, seed=4)
        whole = evaluate_metrics(m, _loader(ds, 128, m), topk=5, progress=False)
        sampler = DistributedIndexSampler(len(ds), ws, rank, shuffle=False)
        part = evaluate_metrics(m, _loader(ds, 128, m, sampler=sampler), topk=5, comm_group=dist.group.WORLD,
                                progress=False)
        assert part.samples == whole.samples == 1003
        assert (part.top1, part.topk, part.k) == (whole.top1, whole.topk, 5), (part, whole)  # the counts: exact
        assert _close(part.loss, whole.loss), (part.loss, whole.loss)
        both = [None] * ws
        dist.all_gather_object(both, tuple(part))
        assert both[0] == both[1], both
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_sharded_evaluation_over_two_gloo_processes():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    try:
        mp.spawn(_gloo_worker, args=(2, free_port(), q), nprocs=2, join=True)
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get())
        raise AssertionError("\n".join(msgs) or "worker failed")


def _train(tmp_path, tag, **validation):
    m = _mlp(seed=11)
    train = _loader(synthetic_cifar(256, seed=6), 64, m, train=True)
    o = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    sched = one_cycle(o, len(train))
    metrics = MetricsWriter(str(tmp_path / f"{tag}.jsonl"))
    if validation:
        validation["val_data"] = _loader(synthetic_cifar(100, seed=7), 64, m)
        validation["best_path"] = str(tmp_path / f"{tag}_best.pt")
    tr = Trainer(m, train, o, 0, 100, sched, metrics=metrics, ckpt_path=str(tmp_path / f"{tag}.pt"), **validation)
    tr.train(2)
    metrics.close()
    f = flat_of(m)
    return m, f.master.clone(), {k: v.clone() for k, v in f.state_tensors.items()}, tr


def test_trainer_validation_leaves_training_bitwise_alone(tmp_path, capsys):
    _, w0, s0, _ = _train(tmp_path, "plain")
    plain_out = capsys.readouterr().out
    m, w1, s1, tr = _train(tmp_path, "val", eval_every=1, topk=5, save_best=True)
    val_out = capsys.readouterr().out
    assert torch.equal(w0, w1)
    assert s0.keys() == s1.keys() and s0 and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert "Validation" not in plain_out
    lines = [ln for ln in val_out.splitlines() if "Validation" in ln]
    assert len(lines) == 2 and all(
        re.fullmatch(rf"Epoch {e} \| Validation loss=\d+\.\d{{4}} top-1=\d+\.\d\d% top-5=\d+\.\d\d%", ln)
        for e, ln in enumerate(lines)), val_out
    recs = [json.loads(ln) for ln in open(tmp_path / "val.jsonl")]
    ev = [r for r in recs if r.get("event") == "eval"]
    assert [r["epoch"] for r in ev] == [0, 1]
    assert all({"val_loss", "val_top1", "val_topk", "k", "samples", "seconds"} <= r.keys() for r in ev)
    assert all(r["k"] == 5 and r["samples"] == 100 for r in ev)
    assert not [r for r in map(json.loads, open(tmp_path / "plain.jsonl")) if r.get("event") == "eval"]
    # the best checkpoint: the reference's format (a plain state dict), and the weights of the best validation
    best = torch.load(tmp_path / "val_best.pt", weights_only=True)
    twin = MLP(hidden=64)
    twin.load_state_dict(best)
    assert tr.best_top1 == max(r["val_top1"] for r in ev)
    if ev[1]["val_top1"] > ev[0]["val_top1"]:
        assert all(torch.equal(v, m.state_dict()[k]) for k, v in best.items())
    assert not os.path.exists(tmp_path / "plain_best.pt")


def _cli(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "2", "5", *extra, "--device", "cpu", "--model", "mlp",
           "--data", "synthetic", "--hidden", "64", "--batch_size", "64", "--train_size", "128", "--test_size", "70",
           "--eval_batch", "32"]
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)


VAL = r"Epoch \d+ \| Validation loss=\d+\.\d{4} top-1=\d+\.\d\d%"


def test_cli_prints_the_validation_lines_only_with_the_flags(tmp_path):
    r = _cli(tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Validation" not in r.stdout and "top-" not in r.stdout, r.stdout
    assert len(re.findall(r"fp32 model has accuracy=\d+\.\d\d%", r.stdout)) == 1
    assert not os.path.exists(tmp_path / "checkpoint_best.pt")
    r = _cli(tmp_path, "--eval_every", "1", "--topk", "3", "--save_best", "--ema_decay", "0.9", "--metrics", "m.jsonl")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len([ln for ln in lines if re.fullmatch(VAL + r" top-3=\d+\.\d\d%", ln)]) == 2, r.stdout
    assert len([ln for ln in lines if re.fullmatch(VAL.replace("Validation", "EMA validation") + r" top-3=\d+\.\d\d%",
                                                   ln)]) == 2, r.stdout
    for name in ("fp32", "EMA"):
        i = [j for j, ln in enumerate(lines) if re.fullmatch(rf"{name} model has accuracy=\d+\.\d\d%", ln)]
        assert len(i) == 1 and re.fullmatch(rf"{name} model has top-3 accuracy=\d+\.\d\d%", lines[i[0] + 1]), r.stdout
    ev = [rec for rec in map(json.loads, open(tmp_path / "m.jsonl")) if rec.get("event") == "eval"]
    assert len(ev) == 2 and all("ema_val_top1" in rec and rec["samples"] == 70 for rec in ev)
    sd = torch.load(tmp_path / "checkpoint_best.pt", weights_only=True)
    assert list(sd) == list(torch.load(tmp_path / "checkpoint.pt", weights_only=True))
    r = _cli(tmp_path, "--save_best")
    assert r.returncode != 0 and "--save_best needs --eval_every" in r.stderr
