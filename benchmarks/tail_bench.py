#!/usr/bin/env python3
"""The published ResNet-9 tail, Cutout and flip TTA against their siblings, at batch 512.

    python benchmarks/tail_bench.py [--section pool|augment|step|eval|all] [--batch 512] [--windows 9] [--out FILE]

``pool``     gmaxpool forward / backward against avgpool forward / backward at [N, 4, 4, 512], bf16 and fp32;
``augment``  the batch's augment launch with ``cutout=8`` against without, nhwc8_bf16 and flat_bf16, plain and mixed
             (Mixup + CutMix on every batch);
``step``     a captured ``Trainer`` step of ``--model resnet9`` with the published tail (max, 0.125) against the
             average tail, bf16 and fp32;
``eval``     ``evaluate_metrics`` over 10000 images with and without ``tta_flip`` (ResNet-9 bf16, published tail).

HIP events around windows of back-to-back calls, the candidates taking turns window by window; median / lowest /
highest window per candidate and the sibling's own spread.  Kernel times come from a trace of their own
(``rocprofv3 --kernel-trace --stats -- python benchmarks/tail_bench.py --section pool``).  One JSON line per
measurement.
"""
import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.resnet_bench import stats, windows  # noqa: E402

LINES = []


def emit(**kw):
    s = json.dumps(kw)
    LINES.append(s)
    print(s, flush=True)


def compare(section, new, old, w, **kw):
    a, b = stats(w[new]), stats(w[old])
    emit(section=section, **kw, **{new: a, old: b},
         sibling_spread_pct=round(100 * (b["max_us"] - b["min_us"]) / b["median_us"], 1),
         ratio=round(a["median_us"] / b["median_us"], 3))


def pool_section(a):
    from ddpx.ops import conv as K
    from ddpx.ops import f32
    dev = torch.device("cuda")
    N, H, C = a.batch, 4, 512
    for dtype, ops in (("bf16", K), ("fp32", f32)):
        dt = torch.bfloat16 if dtype == "bf16" else torch.float32
        torch.manual_seed(0)
        x = torch.randn(N, H, H, C, device=dev).to(dt)
        g = torch.randn(N, C, device=dev).to(dt)
        w = windows({"gmaxpool": lambda: ops.gmaxpool(x, 0.125), "avgpool": lambda: ops.avgpool(x)}, a.windows,
                    a.calls)
        compare("pool", "gmaxpool", "avgpool", w, op="forward", shape=[N, H, H, C], dtype=dtype)
        w = windows({"gmaxpool": lambda: ops.gmaxpool_backward(g, x, 0.125),
                     "avgpool": lambda: ops.avgpool_backward(g, N, H, H, C)}, a.windows, a.calls)
        compare("pool", "gmaxpool", "avgpool", w, op="backward", shape=[N, H, H, C], dtype=dtype)


def augment_section(a):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.data.mix import MixConfig
    dev = torch.device("cuda")
    N = a.batch
    ds = synthetic_cifar(N * 4, seed=1)
    for layout in ("nhwc8_bf16", "flat_bf16"):
        for mixed in (False, True):
            mix = MixConfig(0.2, 1.0) if mixed else None
            ld = {c: DeviceLoader(ds, N, dev, train=True, layout=layout, seed=0, mix=mix, cutout=c) for c in (0, 8)}
            idx = ld[0]._epoch_indices()[:N]
            x, y = ld[0].make_batch(idx, 0)
            bufs = {c: (torch.empty_like(x), torch.empty_like(y)) for c in (0, 8)}
            w = windows({"cutout8": lambda: ld[8].make_batch(idx, 1, *bufs[8]),
                         "plain": lambda: ld[0].make_batch(idx, 1, *bufs[0])}, a.windows, a.calls)
            compare("augment", "cutout8", "plain", w, layout=layout, mixed=mixed, batch=N)


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
        graphs = {}
        keep = []
        for name, kw in (("max_0.125", dict(tail="max", tail_scale=0.125)), ("avg", {})):
            torch.manual_seed(0)
            model = build_model("resnet9", dtype=dtype, device=dev, kernels="native", **kw)
            ddpx.prepare_model(model, dev)
            opt = SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4, capturable=True,
                      fused_backward=True)
            loader = DeviceLoader(synthetic_cifar(N * 6, seed=1), N, dev, train=True, layout=model.input_layout(dev),
                                  seed=2)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
            tr = Trainer(model, loader, opt, 0, 10 ** 9, sched, graph=True, graph_warmup=2,
                         ckpt_path=os.path.join(a.tmp, "tail_bench_ckpt.pt"))
            tr.train(1)
            torch.cuda.synchronize()
            if tr._graph is None:
                raise RuntimeError(f"capture failed: {tr.graph_error}")
            graphs[name] = tr._graph
            keep.append((model, opt, loader, tr))
        w = windows(graphs, a.windows, a.step_calls)
        compare("step", "max_0.125", "avg", w, model="resnet9", batch=N, dtype=dtype)


def eval_section(a):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.models import build_model
    from ddpx.train.evaluate import evaluate_metrics
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = build_model("resnet9", dtype="bf16", device=dev, kernels="native", tail="max", tail_scale=0.125)
    ddpx.prepare_model(m, dev)
    data = DeviceLoader(synthetic_cifar(10000, seed=1), a.batch, dev, train=False, layout=m.input_layout(dev))
    w = windows({"tta_flip": lambda: evaluate_metrics(m, data, progress=False, tta_flip=True),
                 "plain": lambda: evaluate_metrics(m, data, progress=False)}, a.windows, 1, warmup=1)
    compare("eval", "tta_flip", "plain", w, model="resnet9", dtype="bf16", images=10000, batch=a.batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["pool", "augment", "step", "eval", "all"])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2000,
                    help="kernel calls per window (about 10 us each: windows of ~20 ms, not of the scheduler's noise)")
    ap.add_argument("--step_calls", type=int, default=10, help="training steps per window")
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name, fn in (("pool", pool_section), ("augment", augment_section), ("step", step_section),
                     ("eval", eval_section)):
        if a.section in (name, "all"):
            fn(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
