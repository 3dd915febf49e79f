#!/usr/bin/env python3
"""Optimizer-traffic microbenchmark for LAMB (csrc/kernels/lamb.hip), modelled on lars_bw.py.

Times (HIP events, median over reps of `inner` back-to-back calls), over the toy MLP's store (29.4 M) and the wide
MLP's (319 M), with fp32 and bf16 gradients, in ONE job so the numbers share a machine and its neighbours, the
candidates taking turns:
  * the moments pass (ddpx_lamb_moments: 24 B per weight, 22 with bf16 gradients), with plain and with non-temporal
    m / v stores (the default was chosen from this table),
  * the totals + trust launches (ddpx_lars_segment_reduce + ddpx_lars_trust on the partials: a few KB),
  * the apply pass (ddpx_lamb_apply: 18 B per weight), with 1, 2, 4 and 8 workgroups per chunk,
  * the three in sequence, as a step issues them (42 / 40 B per weight): the apply pass then reads the m and v the
    moments pass has just written,
  * ddpx_adamw_flat over the same buffers (30 / 28 B per weight),
  * a torch copy of each pass's bytes (bandwidth reference: half read, half written),
and prints time, achieved TB/s and each pass's rate relative to the copy of its own bytes.
`--steps`: also a whole captured Trainer step of `--model mlp --dtype bf16` (batch 512) with `--optimizer lamb`
next to `--optimizer adamw`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.adamw_bw import mlp_shapes, timeit_many  # noqa: E402
from ddpx.ops.elementwise import adamw_advance_, adamw_flat_  # noqa: E402
from ddpx.ops.lamb import LambPlan  # noqa: E402
from ddpx.runtime import native  # noqa: E402
from ddpx.runtime.flat_params import FlatParams  # noqa: E402

HP = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)


class _Shapes(torch.nn.Module):
    def __init__(self, shapes, dev):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, device=dev) * 0.01) for s in shapes])


def kernel_bench(name, shapes, dev, reps):
    lib = native.kernels()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    bc = torch.ones(2, device=dev)
    adamw_advance_(counter, bc, *HP["betas"])
    stores = {}
    for tag, gd in (("f32grad", torch.float32), ("bf16grad", torch.bfloat16)):
        flat = FlatParams(_Shapes(shapes, dev), grad_dtype=gd, shadow_dtype=torch.bfloat16)
        flat.grad.copy_((torch.randn(flat.total, device=dev) * 1e-3).to(gd))
        stores[tag] = (flat, LambPlan(flat), torch.zeros(flat.total, device=dev), torch.zeros(flat.total, device=dev))
    n = stores["f32grad"][0].total
    lr = torch.full((), 1e-7, device=dev)  # (tiny: thousands of timed updates must not blow the weights up)
    copies = {}
    src = torch.empty(n * 42 // 8 // 2, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    for b in (18, 22, 24, 28, 30, 40, 42):  # b / 2 bytes read + b / 2 written per weight
        copies[b] = (src[:n * b // 8 // 2], dst[:n * b // 8 // 2])

    def moments(plan, m, v, nt):
        def run():
            lib.ddpx_lamb_set_nt(nt)
            plan.moments(0, m, v, bc, **HP)
        return run

    def totals(plan):
        def run():
            plan.reduce()
            plan.trust()
        return run

    def apply(flat, plan, m, v, split):
        def run():
            lib.ddpx_lamb_set_split(split)
            plan.apply(0, flat.total, lr, m, v, bc, HP["eps"], HP["weight_decay"])
        return run

    def whole(flat, plan, m, v, nt, split):
        a, b, c = moments(plan, m, v, nt), totals(plan), apply(flat, plan, m, v, split)

        def run():
            a()
            b()
            c()
        return run

    default_split, default_nt = lib.ddpx_lamb_set_split(0), lib.ddpx_lamb_set_nt(-1)
    fns, bpp = {}, {}
    for b, (src, dst) in copies.items():
        fns[f"copy_{b}Bpp"] = (lambda s, d: (lambda: d.copy_(s)))(src, dst)
        bpp[f"copy_{b}Bpp"] = b
    for tag, (flat, plan, m, v) in stores.items():
        g16 = tag == "bf16grad"
        for nt in (0, 1):
            fns[f"lamb_moments_{tag}_nt{nt}"] = moments(plan, m, v, nt)
            bpp[f"lamb_moments_{tag}_nt{nt}"] = 22 if g16 else 24
            fns[f"lamb_step_{tag}_nt{nt}"] = whole(flat, plan, m, v, nt, default_split)
            bpp[f"lamb_step_{tag}_nt{nt}"] = 40 if g16 else 42
        fns[f"lamb_totals_trust_{tag}"] = totals(plan)
        bpp[f"lamb_totals_trust_{tag}"] = 0
        fns[f"lamb_apply_{tag}"] = apply(flat, plan, m, v, default_split)
        bpp[f"lamb_apply_{tag}"] = 18
        fns[f"ddpx_adamw_flat_{tag}"] = (lambda f, mm, vv: (lambda: adamw_flat_(
            f.master, mm, vv, f.grad, f.shadow, lr, bc, None, *HP["betas"], HP["eps"], HP["weight_decay"])))(flat, m, v)
        bpp[f"ddpx_adamw_flat_{tag}"] = 28 if g16 else 30
    flat, plan, m, v = stores["f32grad"]
    for split in (1, 2, 4, 8):
        fns[f"lamb_apply_f32grad_split{split}"] = apply(flat, plan, m, v, split)
        bpp[f"lamb_apply_f32grad_split{split}"] = 18
    t = timeit_many(fns, reps=reps)
    lib.ddpx_lamb_set_split(default_split)
    lib.ddpx_lamb_set_nt(default_nt)
    res = {"n": n, "chunks": plan.n_chunks, "default_split": default_split, "default_nt": default_nt}
    for k, (med, lo, hi) in t.items():
        res[k] = {"us": med, "min_us": lo, "max_us": hi, "bytes_per_weight": bpp[k],
                  "TBps": round(n * bpp[k] / med / 1e6, 3)}
    for k in list(t):
        b = bpp[k]
        if not k.startswith("copy_") and b:
            res[k]["rate_vs_copy_of_its_bytes"] = round(res[f"copy_{b}Bpp"]["us"] / res[k]["us"], 3)
    print(name, json.dumps(res), flush=True)
    return res


def step_bench(dev, reps, inner=50):
    """Whole captured training steps through ``Trainer._run_batch`` (batch 512, synthetic batch), the candidates
    taking turns."""
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.app import build_model_and_optimizer, build_parser
    from ddpx.train.trainer import Trainer
    common = ["1", "1", "--model", "mlp", "--dtype", "bf16", "--data", "synthetic", "--graph"]
    variants = {"lamb": ["--optimizer", "lamb"], "adamw": ["--optimizer", "adamw"]}
    x = torch.rand(512, 3072, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 10, (512,), device=dev)
    fns, keep = {}, []
    for name, extra in variants.items():
        args = build_parser("lamb_bw").parse_args(common + extra)
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
    res["lamb_minus_adamw_us"] = round(res["lamb"]["us"] - res["adamw"]["us"], 2)
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
        raise SystemExit("lamb_bw: needs a GPU (a CPU timing says nothing about the kernel)")
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
