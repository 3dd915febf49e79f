#!/usr/bin/env python3
"""Optimizer-traffic microbenchmark for the fused flat AdamW (csrc/kernels/adamw.hip), modelled on sgd_bw.py.

Times (HIP events, median over reps of `inner` back-to-back calls), over the toy MLP's parameter count (29.4 M)
and the wide MLP's (319 M), in ONE job so the numbers share a machine and its neighbours:
  * a torch copy of the same bytes (bandwidth reference),
  * ddpx_adamw_flat with fp32 and bf16 gradients: 30 / 28 B per weight (16 read; 4 + 4 + 4 + 2 written),
  * ddpx_sgd_flat over the same store (18 B per weight): the flat stream's known rate,
  * torch.optim.AdamW(fused=True) and (foreach=True) over the same fp32 tensors, as one flat tensor and as the
    MLP's six parameters (views of the same buffers); torch writes no bf16 copy: 28 B per weight,
alternating ours and torch's per round, and prints time, achieved TB/s and the ratio.
`--steps`: also a whole captured Trainer step of `--model mlp --dtype bf16` (batch 512) with `--optimizer adamw`
next to `--optimizer sgd --no_fused_optimizer` (and the default fused-backward SGD for scale).
`--groups`: instead, the table-driven updates of optimizers with parameter groups (ddpx_adamw_flat_hyper and
ddpx_sgd_flat_chunks over a chunk table, rows as `--no_decay_1d` makes them) against ddpx_adamw_flat / ddpx_sgd_flat
over the same store's buffers, windows interleaved, with the flat kernels' own window-to-window spread; with
`--steps` a captured Trainer step of `--optimizer adamw --no_decay_1d` next to `--optimizer adamw`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddpx.ops.elementwise import adamw_advance_, adamw_flat_, sgd_flat_  # noqa: E402

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000 / inner


def timeit_many(fns, reps=15, inner=10):
    """{name: (median, min, max) µs per call}: the candidates take turns, one window each per round, so a noisy
    neighbour or a clock change hits all of them alike."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(window(fn, inner))
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (round(v[len(v) // 2], 2), round(v[0], 2), round(v[-1], 2))
    return out


def mlp_shapes(hidden, layers=3, in_features=3072, classes=10):
    dims = [in_features] + [hidden] * (layers - 1) + [classes]
    shapes = []
    for a, b in zip(dims[:-1], dims[1:]):
        shapes += [(b, a), (b,)]
    return shapes


def kernel_bench(name, shapes, dev, reps):
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        k = 1
        for d in s:
            k *= d
        n = -(-(n + k) // 64) * 64
    p = torch.randn(n, device=dev) * 0.01
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    g32 = torch.randn(n, device=dev) * 1e-3
    g16 = g32.to(torch.bfloat16)
    lr = torch.full((), HP["lr"], device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    bc = torch.ones(2, device=dev)
    adamw_advance_(counter, bc, *HP["betas"])
    args = (lr, bc, None, *HP["betas"], HP["eps"], HP["weight_decay"])
    # torch over the same buffers: one flat parameter, and the model's parameters as views of it
    tp = torch.nn.Parameter(p.clone())
    tp.grad = g32
    views = []
    tp6 = p.clone()
    for s, o in zip(shapes, offs):
        k = 1
        for d in s:
            k *= d
        q = torch.nn.Parameter(tp6[o:o + k].view(s))
        q.grad = g32[o:o + k].view(s)
        views.append(q)
    t_fused1 = torch.optim.AdamW([tp], fused=True, **HP)
    t_each1 = torch.optim.AdamW([tp], foreach=True, **HP)
    t_fused6 = torch.optim.AdamW(views, fused=True, **HP)
    t_each6 = torch.optim.AdamW(views, foreach=True, **HP)
    src = torch.empty(n * 30 // 8 // 2, dtype=torch.float64, device=dev)  # 15 B read + 15 B written per weight
    dst = torch.empty_like(src)
    mom = torch.zeros(n, device=dev)
    fns = {
        "copy_30Bpp": lambda: dst.copy_(src),
        "ddpx_adamw_f32grad": lambda: adamw_flat_(p, m, v, g32, sh, *args),
        "ddpx_adamw_bf16grad": lambda: adamw_flat_(p, m, v, g16, sh, *args),
        "ddpx_sgd_f32grad": lambda: sgd_flat_(p, mom, g32, sh, lr, 0.9, 5e-4),
        "torch_fused_flat": t_fused1.step,
        "torch_fused_params": t_fused6.step,
        "torch_foreach_flat": t_each1.step,
        "torch_foreach_params": t_each6.step,
    }
    bpp = {"copy_30Bpp": 30, "ddpx_adamw_f32grad": 30, "ddpx_adamw_bf16grad": 28, "ddpx_sgd_f32grad": 18,
           "torch_fused_flat": 28, "torch_fused_params": 28}
    t = timeit_many(fns, reps=reps)
    res = {"n": n}
    for k, (med, lo, hi) in t.items():
        res[k] = {"us": med, "min_us": lo, "max_us": hi}
        if k in bpp:
            res[k]["bytes_per_weight"] = bpp[k]
            res[k]["TBps"] = round(n * bpp[k] / med / 1e6, 3)
    ours = res["ddpx_adamw_f32grad"]["us"]
    res["torch_fused_params_over_ddpx"] = round(res["torch_fused_params"]["us"] / ours, 3)
    res["torch_fused_flat_over_ddpx"] = round(res["torch_fused_flat"]["us"] / ours, 3)
    res["torch_foreach_params_over_ddpx"] = round(res["torch_foreach_params"]["us"] / ours, 3)
    print(name, json.dumps(res), flush=True)
    return res


def groups_bench(name, shapes, dev, reps, kinds=("adamw", "sgd")):
    """The table-driven update against its flat sibling over ONE store's buffers (fp32 and bf16 gradients): the
    flat kernel runs over the whole store, the table-driven one over its chunk table (the parameters; the padding
    between them is a few elements).  Rows: weight decay 0 on the 1-D parameters, lr_mul 1 (``decay_groups``)."""
    from ddpx.ops.lars import PidChunkPlan
    from ddpx.optim.flat import Hyper
    from ddpx.runtime.flat_params import FlatParams

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, device=dev) * 0.01)
                                              for s in shapes])
    res = {}
    for gd in (torch.float32, torch.bfloat16):
        flat = FlatParams(Net(), grad_dtype=gd, shadow_dtype=torch.bfloat16)
        n = flat.total
        flat.grad.copy_((torch.randn(n, device=dev) * 1e-3).to(gd))
        m, v, mom = (torch.zeros(n, device=dev) for _ in range(3))
        lr = torch.full((), HP["lr"], device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        bc = torch.ones(2, device=dev)
        adamw_advance_(counter, bc, *HP["betas"])
        wd = [0.0 if p.dim() <= 1 else HP["weight_decay"] for p in flat.params]
        table = torch.tensor([(1.0, w) for w in wd], dtype=torch.float32).to(dev)
        hyper = Hyper([0] * len(wd), [1.0] * len(wd), wd, False, table)
        plan = PidChunkPlan(flat)
        p, g, sh = flat.master, flat.grad, flat.shadow
        fns, bpp = {}, {}
        if "adamw" in kinds:
            fns["adamw_flat"] = lambda: adamw_flat_(p, m, v, g, sh, lr, bc, None, *HP["betas"], HP["eps"],
                                                    HP["weight_decay"])
            fns["adamw_hyper"] = lambda: plan.adamw_update(0, n, hyper, lr, m, v, bc, *HP["betas"], HP["eps"])
            bpp["adamw"] = 26 + g.element_size()
        if "sgd" in kinds:
            fns["sgd_flat"] = lambda: sgd_flat_(p, mom, g, sh, lr, 0.9, 5e-4)
            fns["sgd_hyper"] = lambda: plan.sgd_update(0, n, hyper, lr, 0.9, momentum_buf=mom)
            bpp["sgd"] = 14 + g.element_size()
        t = timeit_many(fns, reps=reps)
        row = {"n": n, "chunks": plan.n_chunks}
        for k, (med, lo, hi) in t.items():
            row[k] = {"us": med, "min_us": lo, "max_us": hi, "TBps": round(n * bpp[k.split("_")[0]] / med / 1e6, 3)}
        for kind in bpp:
            f, h = row[kind + "_flat"], row[kind + "_hyper"]
            row[kind + "_hyper_over_flat"] = round(h["us"] / f["us"], 4)
            row[kind + "_flat_spread"] = round((f["max_us"] - f["min_us"]) / f["us"], 4)
        res[str(gd)[6:] + "_grad"] = row
        del flat, plan, fns
    print(name, json.dumps(res), flush=True)
    return res


def step_bench(dev, reps, inner=50, groups=False):
    """Whole captured training steps through ``Trainer._run_batch`` (batch 512, synthetic batch), the candidates
    taking turns."""
    from ddpx.optim.schedule import one_cycle
    from ddpx.train.app import build_model_and_optimizer, build_parser
    from ddpx.train.trainer import Trainer
    common = ["1", "1", "--model", "mlp", "--dtype", "bf16", "--data", "synthetic", "--graph"]
    variants = {"adamw": ["--optimizer", "adamw"],
                "sgd_unfused": ["--optimizer", "sgd", "--no_fused_optimizer"],
                "sgd_fused_backward": ["--optimizer", "sgd"]}
    if groups:
        variants = {"adamw": ["--optimizer", "adamw"],
                    "adamw_no_decay_1d": ["--optimizer", "adamw", "--no_decay_1d"],
                    "sgd_unfused": ["--optimizer", "sgd", "--no_fused_optimizer"],
                    "sgd_no_decay_1d": ["--optimizer", "sgd", "--no_decay_1d"]}
    x = torch.rand(512, 3072, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 10, (512,), device=dev)
    fns, keep = {}, []
    for name, extra in variants.items():
        args = build_parser("adamw_bw").parse_args(common + extra)
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
    res["adamw_minus_sgd_unfused_us"] = round(res["adamw"]["us"] - res["sgd_unfused"]["us"], 2)
    if groups:
        for k in ("adamw", "sgd"):
            base = res["adamw" if k == "adamw" else "sgd_unfused"]
            res[k + "_no_decay_1d_over_one_group"] = round(res[k + "_no_decay_1d"]["us"] / base["us"], 4)
            res[k + "_one_group_spread"] = round((base["max_us"] - base["min_us"]) / base["us"], 4)
    print("trainer_step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", action="store_true", help="also time whole Trainer steps")
    ap.add_argument("--no_wide", action="store_true")
    ap.add_argument("--groups", action="store_true", help="time the table-driven (parameter-group) updates instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_bw: needs a GPU (a CPU timing says nothing about the kernel)")
    dev = torch.device("cuda")
    bench = groups_bench if a.groups else kernel_bench
    res = {"mlp": bench("mlp", mlp_shapes(4096), dev, a.reps)}
    if not a.no_wide:
        res["mlp_wide"] = bench("mlp_wide", mlp_shapes(16384), dev, a.reps)
    if a.steps:
        res["trainer_step"] = step_bench(dev, a.reps, groups=a.groups)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
