#!/usr/bin/env python3
"""Validation cost, in three sections (``--section``), each one job with its candidates' windows interleaved.

``kernel``    ``ddpx_eval_metrics`` at M = 512, C = 10 / 100 / 128, k = 5 against ``ddpx_accuracy`` alone and against
              stock ``F.cross_entropy(reduction="sum")`` + ``topk`` on the same fp32 logits, all three accumulating on
              the device (``adamw_bw.timeit_many``: HIP events, median over reps of `inner` back-to-back calls).
              Run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the kernel times.
``evaluate``  a whole ``evaluate()`` of a 10000-image synthetic test set, batch 512, toy MLP and VGG bf16: host clock
              around the call, which ends in its device read.  It imports ``ddpx`` from ``--tree`` (default: this
              checkout), so the same script times a build of another commit; ``evaluate_metrics`` is timed too where
              the tree has it.  Alternate the trees' runs in one job.
``epoch``     ``evaluate_metrics`` of the 10000 images against one training epoch of 50000 (batch 512, captured step)
              at world size 1, and from the two per-sample times the evaluation's share of an epoch at N ranks with
              and without ``--shard_eval``.  The N-rank shares are arithmetic on the measured per-sample times, not
              measurements.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, K_TOP = 512, 5
CLASSES = (10, 100, 128)
TEST_N, TRAIN_N, BATCH = 10000, 50000, 512


def section_kernel(dev, a):
    from benchmarks.adamw_bw import timeit_many
    from ddpx.ops.head import EvalAccumulator, accuracy_count, eval_metrics
    fns, keep = {}, []
    for C in a.classes:
        g = torch.Generator().manual_seed(C)
        z = (torch.randn(M, C, generator=g) * 3).to(dev)
        t = torch.randint(0, C, (M,), generator=g).to(dev)
        acc = EvalAccumulator(dev)
        correct = torch.zeros((), dtype=torch.int32, device=dev)
        loss, h1, hk = (torch.zeros((), device=dev, dtype=dt) for dt in (torch.float64, torch.int64, torch.int64))

        def stock(z=z, t=t, loss=loss, h1=h1, hk=hk):
            loss.add_(F.cross_entropy(z, t, reduction="sum"))
            top = z.topk(K_TOP, dim=1).indices == t[:, None]
            h1.add_(top[:, 0].sum())
            hk.add_(top.sum())

        def stock_top1(z=z, t=t, loss=loss, h1=h1):
            loss.add_(F.cross_entropy(z, t, reduction="sum"))
            h1.add_((z.argmax(1) == t).sum())
        fns[f"eval_metrics_c{C}"] = lambda z=z, t=t, acc=acc: eval_metrics(z, t, acc, K_TOP)
        fns[f"accuracy_c{C}"] = lambda z=z, t=t, correct=correct: accuracy_count(z, t, correct)
        fns[f"stock_xent_topk_c{C}"] = stock
        fns[f"stock_xent_argmax_c{C}"] = stock_top1
        keep.append((z, t, acc, correct, loss, h1, hk))
    res = {k: {"us": med, "min_us": lo, "max_us": hi}
           for k, (med, lo, hi) in timeit_many(fns, reps=a.reps, inner=a.inner).items()}
    return {"M": M, "k": K_TOP, "per_call": res}


def _model(dev, name):
    import ddpx
    from ddpx.models import build_model
    torch.manual_seed(0)
    m = build_model(name, dtype="bf16", device=dev, kernels="native")
    ddpx.prepare_model(m, dev)
    return m


def _windows(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # (ends in a device read)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def section_evaluate(dev, a):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.train import evaluate as ev
    out = {"test_images": TEST_N, "batch": BATCH, "tree": a.tree}
    for name in ("mlp", "vgg"):
        m = _model(dev, name)
        data = DeviceLoader(synthetic_cifar(TEST_N, seed=1), BATCH, dev, train=False, layout=m.input_layout(dev))
        fns = {"evaluate": lambda: ev.evaluate(m, data, progress=False)}
        if hasattr(ev, "evaluate_metrics"):
            fns["evaluate_metrics_top5"] = lambda: ev.evaluate_metrics(m, data, topk=K_TOP, progress=False)
        rounds = {k: [] for k in fns}
        for _ in range(a.rounds):  # the candidates take turns
            for k, fn in fns.items():
                rounds[k].append(_windows(fn, a.reps))
        out[name] = {k: {"ms": round(statistics.median(r["ms"] for r in v), 4),
                         "min_ms": min(r["min_ms"] for r in v), "max_ms": max(r["max_ms"] for r in v)}
                     for k, v in rounds.items()}
        out[name]["accuracy"] = ev.evaluate(m, data, progress=False)
    return out


def section_epoch(dev, a):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.optim import SGD
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.evaluate import evaluate_metrics
    from ddpx.train.trainer import Trainer
    out = {"train_images": TRAIN_N, "test_images": TEST_N, "batch": BATCH}
    for name in ("mlp", "vgg"):
        m = _model(dev, name)
        layout = m.input_layout(dev)
        train = DeviceLoader(synthetic_cifar(TRAIN_N, seed=0), BATCH, dev, train=True, layout=layout)
        test = DeviceLoader(synthetic_cifar(TEST_N, seed=1), BATCH, dev, train=False, layout=layout)
        opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
        tr = Trainer(m, train, opt, 0, 10 ** 9, one_cycle(opt, len(train)), graph=True,
                     ckpt_path=os.path.join(a.tmp, f"eval_bench_{name}.pt"))
        tr.start_epoch = 1  # (no checkpoint: epoch % save_every is never 0)
        tr.train(2)         # warm-up epoch, with the capture
        ep, evs = [], []
        for e in range(a.rounds):  # an epoch and an evaluation take turns
            tr.start_epoch = 2 + e
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train(3 + e)  # (ends in a device synchronise)
            ep.append((time.perf_counter() - t0) * 1e3)
            evs.append(_windows(lambda: evaluate_metrics(m, test, topk=K_TOP, progress=False), a.reps))
        epoch_ms = statistics.median(ep)
        eval_ms = statistics.median(r["ms"] for r in evs)
        t_train, t_eval = epoch_ms / TRAIN_N, eval_ms / TEST_N
        shares = {}
        for n in (1, 8):
            per_rank = t_train * TRAIN_N / n
            full, shard = t_eval * TEST_N, t_eval * TEST_N / n
            shares[f"N{n}"] = {"computed": n != 1, "eval_share_full": round(full / (per_rank + full), 4),
                               "eval_share_sharded": round(shard / (per_rank + shard), 4)}
        out[name] = {"graph": tr._graph is not None, "epoch_ms": round(epoch_ms, 3), "epoch_min_ms": round(min(ep), 3),
                     "epoch_max_ms": round(max(ep), 3), "evaluate_metrics_ms": round(eval_ms, 4),
                     "evaluate_metrics_min_ms": min(r["min_ms"] for r in evs),
                     "evaluate_metrics_max_ms": max(r["max_ms"] for r in evs),
                     "train_us_per_sample": round(t_train * 1e3, 4), "eval_us_per_sample": round(t_eval * 1e3, 4),
                     "eval_share_of_epoch": shares}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", required=True, choices=["kernel", "evaluate", "epoch"])
    ap.add_argument("--tree", default=HERE, help="checkout to import ddpx from (built)")
    ap.add_argument("--out", default=None, help="append the JSON result line to this file")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--classes", type=lambda v: tuple(int(c) for c in v.split(",")), default=CLASSES,
                    help="kernel section: class counts (one per profiler run keeps the trace's kernel names apart)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    a.tree = os.path.abspath(a.tree)
    sys.path.insert(0, a.tree)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda", 0)
    res = {"section": a.section, "tag": a.tag}
    res.update({"kernel": section_kernel, "evaluate": section_evaluate, "epoch": section_epoch}[a.section](dev, a))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
