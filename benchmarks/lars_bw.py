#!/usr/bin/env python3
"""Optimizer-traffic microbenchmark for LARS (csrc/kernels/lars.hip), modelled on adamw_bw.py.

Times (HIP events, median over reps of `inner` back-to-back calls), over the toy MLP's store (29.4 M) and the wide
MLP's (319 M), in ONE job so the numbers share a machine and its neighbours, the candidates taking turns:
  * the norm pass (ddpx_lars_sumsq + ddpx_lars_segment_reduce + ddpx_lars_trust): reads 8 B per weight, 6 with bf16
    gradients, and the sum-of-squares launch alone,
  * ddpx_sgd_flat_chunks with the trust table (rows `ddpx_sgd_flat_lars_*`) with fp32 and bf16 gradients (18 / 16 B
    per weight: 12 / 10 read; 4 + 4 + 2 written), and with 1, 2, 4 and 8 workgroups per chunk (the launch shape was
    chosen from this table),
  * ddpx_sgd_flat over the same buffers (the target: the same bytes with no chunk table),
  * a torch copy of the same bytes (bandwidth reference),
and prints time, achieved TB/s, and the update's gap to ddpx_sgd_flat next to the spread (max - min) of that
kernel's own windows.
`--steps`: also a whole captured Trainer step of `--model mlp --dtype bf16` (batch 512) with `--optimizer lars`
next to `--optimizer sgd --no_fused_optimizer` (and the default fused-backward SGD for scale).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.adamw_bw import mlp_shapes, timeit_many  # noqa: E402
from ddpx.ops.elementwise import sgd_flat_  # noqa: E402
from ddpx.ops.lars import LarsPlan  # noqa: E402
from ddpx.runtime import native  # noqa: E402
from ddpx.runtime.flat_params import FlatParams  # noqa: E402

HP = dict(trust_coef=1e-3, weight_decay=5e-4, eps=1e-8)


class _Shapes(torch.nn.Module):
    def __init__(self, shapes, dev):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, device=dev) * 0.01) for s in shapes])


def kernel_bench(name, shapes, dev, reps):
    lib = native.kernels()
    stores = {}
    for tag, gd in (("f32grad", torch.float32), ("bf16grad", torch.bfloat16)):
        flat = FlatParams(_Shapes(shapes, dev), grad_dtype=gd, shadow_dtype=torch.bfloat16)
        flat.grad.copy_((torch.randn(flat.total, device=dev) * 1e-3).to(gd))
        stores[tag] = (flat, LarsPlan(flat), torch.zeros(flat.total, device=dev))
    n = stores["f32grad"][0].total
    lr = torch.full((), 1e-6, device=dev)  # (tiny: thousands of timed updates must not blow the weights up)
    src = torch.empty(n * 18 // 8 // 2, dtype=torch.float64, device=dev)  # 9 B read + 9 B written per weight
    dst = torch.empty_like(src)

    def norm_pass(plan):
        def run():
            plan.partials(0)
            plan.reduce()
            plan.trust(HP["trust_coef"], HP["weight_decay"], HP["eps"])
        return run

    def update(flat, plan, mom, split):
        def run():
            lib.ddpx_lars_set_split(split)
            plan.update(0, flat.total, lr, 0.9, HP["weight_decay"], momentum_buf=mom)
        return run

    default_split = lib.ddpx_lars_set_split(0)
    fns = {"copy_18Bpp": lambda: dst.copy_(src)}
    bpp = {"copy_18Bpp": 18}
    for tag, (flat, plan, mom) in stores.items():
        g16 = tag == "bf16grad"
        fns[f"lars_norm_pass_{tag}"] = norm_pass(plan)
        fns[f"lars_sumsq_{tag}"] = (lambda pl: (lambda: pl.partials(0)))(plan)
        fns[f"ddpx_sgd_flat_lars_{tag}"] = update(flat, plan, mom, default_split)
        fns[f"ddpx_sgd_flat_{tag}"] = (lambda f, m: (lambda: sgd_flat_(f.master, m, f.grad, f.shadow, lr, 0.9,
                                                                       HP["weight_decay"])))(flat, mom)
        bpp.update({f"lars_norm_pass_{tag}": 6 if g16 else 8, f"lars_sumsq_{tag}": 6 if g16 else 8,
                    f"ddpx_sgd_flat_lars_{tag}": 16 if g16 else 18, f"ddpx_sgd_flat_{tag}": 16 if g16 else 18})
    flat, plan, mom = stores["f32grad"]
    for split in (1, 2, 4, 8):
        fns[f"ddpx_sgd_flat_lars_f32grad_split{split}"] = update(flat, plan, mom, split)
        bpp[f"ddpx_sgd_flat_lars_f32grad_split{split}"] = 18
    stores["f32grad"][1].compute(**HP)
    stores["bf16grad"][1].compute(**HP)
    t = timeit_many(fns, reps=reps)
    lib.ddpx_lars_set_split(default_split)
    res = {"n": n, "chunks": plan.n_chunks, "default_split": default_split}
    for k, (med, lo, hi) in t.items():
        res[k] = {"us": med, "min_us": lo, "max_us": hi, "bytes_per_weight": bpp[k],
                  "TBps": round(n * bpp[k] / med / 1e6, 3)}
    for tag in stores:
        sgd, ours = res[f"ddpx_sgd_flat_{tag}"], res[f"ddpx_sgd_flat_lars_{tag}"]
        res[f"lars_minus_sgd_flat_{tag}_us"] = round(ours["us"] - sgd["us"], 2)
        res[f"sgd_flat_{tag}_spread_us"] = round(sgd["max_us"] - sgd["min_us"], 2)
    print(name, json.dumps(res), flush=True)
    return res


def step_bench(dev, reps, inner=50):
    """Whole captured training steps through ``Trainer._run_batch`` (batch 512, synthetic batch), the candidates
    taking turns."""
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.app import build_model_and_optimizer, build_parser
    from ddpx.train.trainer import Trainer
    common = ["1", "1", "--model", "mlp", "--dtype", "bf16", "--data", "synthetic", "--graph"]
    variants = {"lars": ["--optimizer", "lars"],
                "sgd_unfused": ["--optimizer", "sgd", "--no_fused_optimizer"],
                "sgd_fused_backward": ["--optimizer", "sgd"]}
    x = torch.rand(512, 3072, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 10, (512,), device=dev)
    fns, keep = {}, []
    for name, extra in variants.items():
        args = build_parser("lars_bw").parse_args(common + extra)
        torch.manual_seed(0)
        model, opt = build_model_and_optimizer(args, dev)
        sched = one_cycle(opt, 98)
        tr = Trainer(model, None, opt, 0, 1, sched, graph=True)
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
    res["lars_minus_sgd_unfused_us"] = round(res["lars"]["us"] - res["sgd_unfused"]["us"], 2)
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
        raise SystemExit("lars_bw: needs a GPU (a CPU timing says nothing about the kernel)")
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
