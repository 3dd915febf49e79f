#!/usr/bin/env python3
"""Traffic microbenchmark for the weight-EMA kernel (csrc/kernels/ema.hip), modelled on adamw_bw.py.

Times (HIP events, median over reps of `inner` back-to-back calls), over the toy MLP's parameter count (29.4 M) and
the wide MLP's (319 M), in ONE job with the candidates' windows interleaved:
  * a torch copy of the same bytes, 12 B per weight (6 read, 6 written): the yardstick,
  * ddpx_ema_flat (12 B per weight: 8 read, 4 written) with the default cache policy (plain loads and stores) and
    with the other policies of ddpx_ema_set_nt (non-temporal average with plain weights, all non-temporal),
  * ddpx_ema_flat with w = 0 (a step of `--ema_every K` without update: one scalar load per thread),
  * torch's `Tensor.lerp_` over the same buffers,
and prints time, achieved TB/s, the ratio to the copy and the copy's own window-to-window spread.
`--steps`: also a whole captured Trainer step of `--model mlp --dtype bf16` (batch 512) without an average, with
`--ema_decay 0.999` and with `--ema_decay 0.999 --ema_every 4`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.adamw_bw import mlp_shapes, timeit_many  # noqa: E402
from ddpx.ops.ema import ema_flat_  # noqa: E402
from ddpx.runtime import native  # noqa: E402

BPP = 12
POLICIES = {"ddpx_ema_all_plain": 0, "ddpx_ema_nt_average": 1, "ddpx_ema_all_nt": 3}  # ddpx_ema_set_nt masks


def kernel_bench(name, shapes, dev, reps):
    n = 0
    for s in shapes:
        k = 1
        for d in s:
            k *= d
        n = -(-(n + k) // 64) * 64
    p = torch.randn(n, device=dev) * 0.01
    e = p.clone()
    e2 = p.clone()
    w = torch.full((), 1e-3, device=dev)
    w0 = torch.zeros((), device=dev)
    src = torch.empty(n * BPP // 8 // 2, dtype=torch.float64, device=dev)  # 6 B read + 6 B written per weight
    dst = torch.empty_like(src)
    lib = native.kernels()
    default = lib.ddpx_ema_set_nt(-1)

    def with_nt(mask, weight):
        def fn():
            lib.ddpx_ema_set_nt(mask)
            ema_flat_(e, p, weight)
        return fn

    fns = {
        "copy_12Bpp": lambda: dst.copy_(src),
        "ddpx_ema": with_nt(default, w),
        "ddpx_ema_w0": with_nt(default, w0),
        "torch_lerp": lambda: e2.lerp_(p, w),
    }
    others = {k: m for k, m in POLICIES.items() if m != default}
    for k, m in others.items():
        fns[k] = with_nt(m, w)
    t = timeit_many(fns, reps=reps, inner=50)
    lib.ddpx_ema_set_nt(default)
    res = {"n": n, "default_nt_mask": default}
    for k, (med, lo, hi) in t.items():
        res[k] = {"us": med, "min_us": lo, "max_us": hi}
        if k != "ddpx_ema_w0":
            res[k]["TBps"] = round(n * BPP / med / 1e6, 3)
    c = res["copy_12Bpp"]
    res["copy_spread"] = round((c["max_us"] - c["min_us"]) / c["us"], 4)
    for k in ("ddpx_ema", *others, "torch_lerp"):
        res[k + "_over_copy"] = round(res[k]["us"] / c["us"], 4)
    print(name, json.dumps(res), flush=True)
    return res


def step_bench(dev, reps, inner=50):
    """Whole captured training steps through ``Trainer._run_batch`` (batch 512, synthetic batch), the candidates
    taking turns."""
    from ddpx.optim import WeightEMA
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.app import build_model_and_optimizer, build_parser
    from ddpx.train.trainer import Trainer
    common = ["1", "1", "--model", "mlp", "--dtype", "bf16", "--data", "synthetic", "--graph"]
    variants = {"no_ema": [],
                "ema": ["--ema_decay", "0.999"],
                "ema_every_4": ["--ema_decay", "0.999", "--ema_every", "4"]}
    x = torch.rand(512, 3072, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 10, (512,), device=dev)
    fns, keep = {}, []
    for name, extra in variants.items():
        args = build_parser("ema_bw").parse_args(common + extra)
        torch.manual_seed(0)
        model, opt = build_model_and_optimizer(args, dev)
        ema = WeightEMA(opt, args.ema_decay, every=args.ema_every) if args.ema_decay is not None else None
        sched = one_cycle(opt, 98)
        tr = Trainer(model, None, opt, 0, 1, sched, graph=True, ema=ema)
        tr._device_lr = bool(opt.attach_device_schedule(sched))
        for _ in range(4):  # 2 eager steps, the capture, replays
            tr._run_batch(x, y)
        torch.cuda.synchronize()
        if tr._graph is None:
            raise RuntimeError(f"{name}: the step was not captured ({tr.graph_error})")
        keep.append(tr)
        fns[name] = (lambda t: (lambda: t._run_batch(x, y)))(tr)
    t = timeit_many(fns, reps=reps, inner=inner)
    res = {k: {"us": med, "min_us": lo, "max_us": hi} for k, (med, lo, hi) in t.items()}
    base = res["no_ema"]
    res["no_ema_spread"] = round((base["max_us"] - base["min_us"]) / base["us"], 4)
    for k in ("ema", "ema_every_4"):
        res[k + "_minus_no_ema_us"] = round(res[k]["us"] - base["us"], 2)
    for tr in keep:
        if tr.ema is not None:
            steps, updates = tr.ema.counts()
            res.setdefault("counts", {})["every_%d" % tr.ema.every] = [steps, updates]
    print("trainer_step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", action="store_true", help="also time whole Trainer steps")
    ap.add_argument("--no_wide", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bw: needs a GPU (a CPU timing says nothing about the kernel)")
    dev = torch.device("cuda")
    res = {"mlp": kernel_bench("mlp", mlp_shapes(4096), dev, a.reps)}
    if not a.no_wide:
        res["mlp_wide"] = kernel_bench("mlp_wide", mlp_shapes(16384), dev, a.reps)
    if a.steps:
        res["trainer_step"] = step_bench(dev, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
