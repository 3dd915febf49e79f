#!/usr/bin/env python3
"""Cost of label smoothing / Mixup / CutMix against the entry points they sit beside, in ONE job with the
candidates' windows interleaved (``adamw_bw.timeit_many``: HIP events, median over reps of `inner` back-to-back
calls, every candidate one window per round):

  * ``ddpx_augment`` against ``ddpx_augment_mix`` with every batch Mixup, every batch CutMix, and no batch mixed
    (prob 0: the plain body behind the mixing kernel's draw), at batch 512 in the toy MLP's layout (``flat_bf16``)
    and in VGG's (``nhwc8_bf16``);
  * ``ddpx_head_fwd`` against ``ddpx_head_fwd_soft`` at M = 512, K = 4096 (loss + dlogits, no logits: the training
    launch), with smoothing alone and with smoothing and second labels;
  * ``--steps``: the batch's augment launch plus a whole captured Trainer step of ``--model mlp --dtype bf16``
    (batch 512), without the flags and with ``--label_smoothing 0.1 --mixup_alpha 0.2 --cutmix_alpha 1.0``.

The baseline of every comparison is the old entry point in the same job; each group also reports the baseline's
own window-to-window spread.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.adamw_bw import timeit_many  # noqa: E402
from ddpx.data.datasets import synthetic_cifar  # noqa: E402
from ddpx.data.loader import DeviceLoader  # noqa: E402
from ddpx.data.mix import MixConfig  # noqa: E402
from ddpx.ops.head import head_forward  # noqa: E402
from ddpx.ops.loss import SoftTargets  # noqa: E402

B = 512


def _report(name, t, base, others):
    res = {k: {"us": med, "min_us": lo, "max_us": hi} for k, (med, lo, hi) in t.items()}
    b = res[base]
    res[base + "_spread"] = round((b["max_us"] - b["min_us"]) / b["us"], 4)
    for k in others:
        res[k + "_minus_" + base + "_us"] = round(res[k]["us"] - b["us"], 2)
        res[k + "_over_" + base] = round(res[k]["us"] / b["us"], 4)
    print(name, json.dumps(res), flush=True)
    return res


def augment_bench(layout, dev, reps, inner):
    ds = synthetic_cifar(8192, seed=0)
    variants = {"augment": None, "mix_none": MixConfig(0.2, 1.0, prob=1e-9), "mix_mixup": MixConfig(0.2, 0.0),
                "mix_cutmix": MixConfig(0.0, 1.0)}
    fns, keep = {}, []
    for name, cfg in variants.items():
        ld = DeviceLoader(ds, B, dev, train=True, layout=layout, seed=0, mix=cfg)
        idx = ld._epoch_indices()
        x, y = ld.make_batch(idx[:B], 0)
        state = {"k": 0}

        def fn(ld=ld, idx=idx, x=x, y=y, state=state):
            k = state["k"] = (state["k"] + 1) % 16  # another batch (and draw) every call
            ld.make_batch(idx[k * B:(k + 1) * B], k, out=x, tgt=y)
        keep.append((ld, x, y))
        fns[name] = fn
    return _report("augment_" + layout, timeit_many(fns, reps=reps, inner=inner), "augment",
                   ["mix_none", "mix_mixup", "mix_cutmix"])


def head_bench(dev, reps, inner, M=512, K=4096):
    g = torch.Generator().manual_seed(0)
    h = torch.relu(torch.randn(M, K, generator=g)).to(torch.bfloat16).to(dev)
    w = (torch.randn(10, K, generator=g) * 0.03).to(torch.bfloat16).to(dev)
    b = torch.zeros(10, device=dev)
    a = torch.randint(0, 10, (M,), generator=g).to(dev)
    tb = torch.randint(0, 10, (M,), generator=g).to(dev)
    lam = torch.rand(M, generator=g).to(dev)
    variants = {"head_fwd": None, "head_fwd_soft_smoothing": SoftTargets(None, None, 0.1),
                "head_fwd_soft_mixed": SoftTargets(tb, lam, 0.1)}
    fns = {k: (lambda s=s: head_forward(h, w, b, a, want_logits=False, soft=s)) for k, s in variants.items()}
    return _report("head_fwd", timeit_many(fns, reps=reps, inner=inner), "head_fwd",
                   ["head_fwd_soft_smoothing", "head_fwd_soft_mixed"])


def step_bench(dev, reps, inner=50):
    """The batch's augment launch and a whole captured training step through ``Trainer._run_batch`` (batch 512),
    the candidates taking turns."""
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.app import build_model_and_optimizer, build_parser, mix_config
    from ddpx.train.trainer import Trainer
    common = ["1", "1", "--model", "mlp", "--dtype", "bf16", "--data", "synthetic", "--graph"]
    variants = {"plain": [],
                "soft": ["--label_smoothing", "0.1", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0"]}
    ds = synthetic_cifar(8192, seed=0)
    fns, keep = {}, []
    for name, extra in variants.items():
        args = build_parser("mix_bench").parse_args(common + extra)
        torch.manual_seed(0)
        model, opt = build_model_and_optimizer(args, dev)
        ld = DeviceLoader(ds, B, dev, train=True, layout="flat_bf16", seed=0, mix=mix_config(args))
        idx = ld._epoch_indices()
        x, y = ld.make_batch(idx[:B], 0)
        sched = one_cycle(opt, 98)
        tr = Trainer(model, ld, opt, 0, 1, sched, graph=True, label_smoothing=args.label_smoothing)
        tr._device_lr = bool(opt.attach_device_schedule(sched))
        state = {"k": 0}

        def fn(ld=ld, idx=idx, x=x, y=y, tr=tr, state=state):
            k = state["k"] = (state["k"] + 1) % 16
            ld.make_batch(idx[k * B:(k + 1) * B], k, out=x, tgt=y)
            tr._run_batch(x, y)
        for _ in range(4):  # 2 eager steps, the capture, replays
            fn()
        torch.cuda.synchronize()
        if tr._graph is None:
            raise RuntimeError(f"{name}: the step was not captured ({tr.graph_error})")
        keep.append(tr)
        fns[name] = fn
    return _report("trainer_step", timeit_many(fns, reps=reps, inner=inner), "plain", ["soft"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--steps", action="store_true", help="also time augment + whole captured Trainer steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda")
    res = {"augment_flat_bf16": augment_bench("flat_bf16", dev, a.reps, a.inner),
           "augment_nhwc8_bf16": augment_bench("nhwc8_bf16", dev, a.reps, a.inner),
           "head_fwd": head_bench(dev, a.reps, a.inner)}
    if a.steps:
        res["trainer_step"] = step_bench(dev, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
