#!/usr/bin/env python3
"""ResNet-9: the skip connection fused into the BatchNorm kernels, and a whole training step.

    python benchmarks/resnet_bench.py [--section kernels|step|all] [--batch 512] [--windows 9] [--out FILE]

(a) ``kernels``: on ResNet-9's residual shapes at the given batch ([N,16,16,128] and [N,4,4,512]), bf16 and fp32,
    the fused kernels against the unfused composition they replace:
      forward : bn_apply(..., res=r)              vs  bn_apply(...) followed by a torch add;
      backward: bn_backward(g1, ..., gout2=g2)    vs  a torch add followed by bn_backward(g1 + g2, ...)
    (the backward is the pooled block below the residual block, layer1 / layer3: both gradients at the pooled
    resolution).  HIP events around windows of back-to-back calls, the candidates taking turns window by window;
    median / lowest / highest window per candidate, and the composition's own spread.
(b) ``step``: a captured ``Trainer`` step of ``--model resnet9`` (fused SGD), bf16 and fp32, against the stock
    PyTorch recipe of the same module (torch ops, ``torch.optim.SGD``, autocast bf16 / plain fp32, eager) in the
    same job, windows interleaved.

One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINES = []


def emit(**kw):
    s = json.dumps(kw)
    LINES.append(s)
    print(s, flush=True)


def windows(cands, n_windows, calls, warmup=3):
    """{name: [ms per call of each window]}: the candidates take turns, one window each per round."""
    out = {k: [] for k in cands}
    for k, fn in cands.items():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(n_windows):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / calls)
    return out


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 2), "min_us": round(1e3 * s[0], 2),
            "max_us": round(1e3 * s[-1], 2)}


def kernels_section(a):
    from ddpx.ops import conv as K
    from ddpx.ops import f32
    dev = torch.device("cuda")
    N = a.batch
    for (H, C) in ((16, 128), (4, 512)):
        for dtype in ("bf16", "fp32"):
            dt = torch.bfloat16 if dtype == "bf16" else torch.float32
            torch.manual_seed(0)
            av = torch.rand(C, device=dev) + 0.5
            mean = torch.randn(C, device=dev) * 0.1
            rstd = torch.rand(C, device=dev) + 0.5
            bv = torch.randn(C, device=dev) * 0.2
            # forward: the last block of the residual branch, [N,H,H,C]
            y = torch.randn(N * H * H, C, device=dev).to(dt)
            r = torch.randn(N, H, H, C, device=dev).to(dt)
            if dtype == "bf16":
                fwd = {"fused": lambda: K.bn_apply(y, av, bv, N, H, H, C, res=r),
                       "unfused": lambda: K.bn_apply(y, av, bv, N, H, H, C) + r}
            else:
                fwd = {"fused": lambda: f32.bn_apply(y, av, bv, mean, N, H, H, C, False, res=r),
                       "unfused": lambda: f32.bn_apply(y, av, bv, mean, N, H, H, C, False) + r}
            # backward: the pooled block below, y2 [N,2H,2H,C], gradients [N,H,H,C]
            y2 = torch.randn(N * 4 * H * H, C, device=dev).to(dt)
            g1 = torch.randn(N, H, H, C, device=dev).to(dt)
            g2 = torch.randn(N, H, H, C, device=dev).to(dt)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
            if dtype == "bf16":
                bwd = {"fused": lambda: K.bn_backward(g1, y2, av, bv, mean, rstd, N, 2 * H, 2 * H, C, True, dgamma=dg,
                                                      dbeta=db, gout2=g2),
                       "unfused": lambda: K.bn_backward(g1 + g2, y2, av, bv, mean, rstd, N, 2 * H, 2 * H, C, True,
                                                        dgamma=dg, dbeta=db)}
            else:
                bwd = {"fused": lambda: f32.bn_backward(g1, y2, av, bv, mean, rstd, N, 2 * H, 2 * H, C, True, dg, db,
                                                        g2=g2),
                       "unfused": lambda: f32.bn_backward(g1 + g2, y2, av, bv, mean, rstd, N, 2 * H, 2 * H, C, True,
                                                          dg, db)}
            for which, cands in (("forward", fwd), ("backward", bwd)):
                w = windows(cands, a.windows, a.calls)
                fu, un = stats(w["fused"]), stats(w["unfused"])
                emit(section="kernels", shape=[N, H, H, C], dtype=dtype, op=which, fused=fu, unfused=un,
                     unfused_spread_pct=round(100 * (un["max_us"] - un["min_us"]) / un["median_us"], 1),
                     fused_over_unfused=round(fu["median_us"] / un["median_us"], 3))


def step_section(a):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.models import build_model
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    dev = torch.device("cuda")
    N = a.batch
    for dtype in ("bf16", "fp32"):
        torch.manual_seed(0)
        model = build_model("resnet9", dtype=dtype, device=dev, kernels="native")
        ddpx.prepare_model(model, dev)
        opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True, fused_backward=True)
        loader = DeviceLoader(synthetic_cifar(N * 6, seed=1), N, dev, train=True, layout=model.input_layout(dev),
                              seed=2)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
        tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=True, graph_warmup=2,
                     ckpt_path=os.path.join(a.tmp, "resnet_bench_ckpt.pt"))
        tr.train(1)
        torch.cuda.synchronize()
        if tr._graph is None:
            raise RuntimeError(f"capture failed: {tr.graph_error}")
        stock = build_model("resnet9", dtype=dtype, device=dev, kernels="torch").to(dev)
        stock = stock.to(memory_format=torch.channels_last) if a.channels_last else stock
        sopt = torch.optim.SGD(stock.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        x = torch.rand(N, 3, 32, 32, device=dev)
        if a.channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        t = torch.randint(0, 10, (N,), device=dev)

        def stock_step():
            sopt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
                loss = F.cross_entropy(stock(x).float(), t)
            loss.backward()
            sopt.step()

        w = windows({"native_captured": tr._graph, "stock_eager": stock_step}, a.windows, a.step_calls)
        na, st = stats(w["native_captured"]), stats(w["stock_eager"])
        emit(section="step", model="resnet9", batch=N, dtype=dtype, native_captured=na, stock_eager=st,
             stock_over_native=round(st["median_us"] / na["median_us"], 3), channels_last=bool(a.channels_last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["kernels", "step", "all"])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per window")
    ap.add_argument("--step_calls", type=int, default=10, help="training steps per window")
    ap.add_argument("--channels_last", type=int, default=0, help="stock recipe in channels_last")
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.section in ("kernels", "all"):
        kernels_section(a)
    if a.section in ("step", "all"):
        step_section(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
