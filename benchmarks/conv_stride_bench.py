#!/usr/bin/env python3
"""Stride-2 convolutions (csrc/kernels/conv_igemm_s2.hip, f32_conv_s2.hip) on the ResNet-18 CIFAR transitions.

    python benchmarks/conv_stride_bench.py [--dtype bf16|fp32] [--batch 512] [--windows 9] [--calls 200] [--tiles 0]
                                           [--out FILE]

For 64->128 @32x32, 128->256 @16x16 and 256->512 @8x8 at the given batch: the 3x3 / s2 and 1x1 / s2 forward, data
gradient and weight gradient (fp32 gradient stored; the call allocates its slab buffer and runs the reduce, both in
the figure) against ``torch``'s convolution (the same dtype, channels_last;
``aten.convolution_backward`` with one output requested for each gradient), and the parity-class 3x3 data gradient
against the stride-1 data gradient run over a zero-inserted dy (the insertion itself not timed).  HIP events around
windows of back-to-back calls, the candidates taking turns window by window; median / lowest / highest window.  With
``--tiles 1`` the 3x3 kernels (fp32: the 1x1 too) are also timed on each explicit tile.  ``--dtype fp32`` times ``ddpx.ops.f32``'s
kernels on the same shapes and windows.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.resnet_bench import stats, windows  # noqa: E402

LINES = []


def emit(**kw):
    s = json.dumps(kw)
    LINES.append(s)
    print(s, flush=True)


def spread(st):
    return round(100 * (st["max_us"] - st["min_us"]) / st["median_us"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="calls per window (about 10 ms of work)")
    ap.add_argument("--tiles", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddpx.ops import conv as K
    from ddpx.ops import f32 as K32
    f32 = a.dtype == "fp32"
    dt = torch.float32 if f32 else torch.bfloat16
    dev = torch.device("cuda")
    N = a.batch
    bwd = torch.ops.aten.convolution_backward
    for (H, C, Co) in ((32, 64, 128), (16, 128, 256), (8, 256, 512)):
        Ho = H // 2
        P = N * Ho * Ho
        torch.manual_seed(0)
        x = torch.randn(N, H, H, C, device=dev).to(dt)
        dy = torch.randn(P, Co, device=dev).to(dt)
        xt = x.permute(0, 3, 1, 2)        # NCHW view of NHWC storage: channels_last
        dyt = dy.view(N, Ho, Ho, Co).permute(0, 3, 1, 2)
        for ks in (3, 1):
            w = torch.randn(Co, C, ks, ks, device=dev) * 0.05
            wt = w.to(dt).contiguous(memory_format=torch.channels_last)
            g = torch.empty_like(w)
            if f32 and ks == 3:
                wf, wd = torch.empty(9 * C * Co, device=dev), torch.empty(9 * Co * C, device=dev)
                K32.conv_wprep(w, wf, wd)
                ours = {"fwd": lambda t=-1: K32.conv_s2_fwd(x, wf, Co, stats=True, tile=t),
                        "dgrad": lambda t=-1: K32.conv_s2_dgrad(dy, wd, N, H, H, C, Co, tile=t),
                        "wgrad": lambda t=-1: K32.conv_s2_wgrad(dy, x, Co, C, g, tile=t)}
            elif f32:
                wf = torch.empty(C * Co, device=dev)
                K32.conv1x1_wprep(w, wf)
                ours = {"fwd": lambda t=-1: K32.conv1x1_s2_fwd(x, wf, Co, stats=True, tile=t),
                        "dgrad": lambda t=-1: K32.conv1x1_s2_dgrad(dy, w, N, H, H, C, Co, tile=t),
                        "wgrad": lambda t=-1: K32.conv1x1_s2_wgrad(dy, x, Co, C, g, tile=t)}
            elif ks == 3:
                wf = torch.empty(Co * 9 * C, dtype=torch.bfloat16, device=dev)
                wd = torch.empty_like(wf)
                K.weight_prep(w, wf, wd)
                ours = {"fwd": lambda t=-1: K.conv_s2_fwd(x, wf, Co, stats=True, tile=t),
                        "dgrad": lambda t=-1: K.conv_s2_dgrad(dy, wd, N, H, H, C, Co, tile=t),
                        "wgrad": lambda t=-1: K.conv_s2_wgrad(dy, x, Co, C, out=g, tile=t)}
            else:
                wf = wd = torch.empty(Co * C, dtype=torch.bfloat16, device=dev)
                K.weight_prep_1x1(w, wf, wd)
                ours = {"fwd": lambda: K.conv1x1_s2_fwd(x, wf, Co, stats=True),
                        "dgrad": lambda: K.conv1x1_s2_dgrad(dy, wd, N, H, H, C, Co),
                        "wgrad": lambda: K.conv1x1_s2_wgrad(dy, x, Co, C, out=g)}
            pad = [ks // 2] * 2
            tail = (None, [2, 2], pad, [1, 1], False, [0, 0], 1)
            stock = {"fwd": lambda: torch.nn.functional.conv2d(xt, wt, stride=2, padding=ks // 2),
                     "dgrad": lambda: bwd(dyt, xt, wt, *tail, [True, False, False]),
                     "wgrad": lambda: bwd(dyt, xt, wt, *tail, [False, True, False])}
            for op in ("fwd", "dgrad", "wgrad"):
                cands = {"hip": ours[op], "torch": stock[op]}
                if (ks == 3 or f32) and a.tiles:
                    cands["hip_tile0"] = lambda f=ours[op]: f(0)
                    cands["hip_tile1"] = lambda f=ours[op]: f(1)
                if ks == 3 and op == "dgrad":
                    dyz = torch.zeros(N, H, H, Co, dtype=dt, device=dev)
                    dyz[:, ::2, ::2] = dy.view(N, Ho, Ho, Co)
                    dyz2 = dyz.view(N * H * H, Co)
                    s1 = K32.conv_dgrad if f32 else K.conv_dgrad
                    cands["stride1_zero_inserted"] = lambda: s1(dyz2, wd, N, H, H, C, Co)
                w_ = windows(cands, a.windows, a.calls)
                res = {k: stats(v) for k, v in w_.items()}
                emit(dtype=a.dtype, kernel=f"{ks}x{ks}/s2 {op}", shape=[N, H, H, C, Co],
                     **{k: dict(v, spread_pct=spread(v)) for k, v in res.items()},
                     hip_over_torch=round(res["hip"]["median_us"] / res["torch"]["median_us"], 3))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
