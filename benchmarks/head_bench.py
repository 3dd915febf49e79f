#!/usr/bin/env python3
"""The classifier head at 10, 100 and 128 classes, in ONE job with the candidates' windows interleaved
(``adamw_bw.timeit_many``: HIP events, median over reps of `inner` back-to-back calls, every candidate one window
per round).  M = 512, K in {512, 4096}; per K one group each for

  * forward (loss + dlogits, no logits: the training launch): ``ddpx_head_fwd`` at C = 10 (one class tile, the
    baseline), 100 and 128 (7 and 8 class tiles), and stock ``F.linear + F.cross_entropy`` under bf16 autocast
    (forward only) at each C;
  * backward with stored gradients (dW, db, dH, previous-layer bias): ``ddpx_head_bwd`` at C = 10 (the 10-class
    kernel), 100 and 128 (the exact-f32 MFMA kernel), and stock autograd's backward of the same loss at each C;
  * backward with the SGD update fused (momentum 0.9), native only;
  * the fp32 head (``f32.head_forward`` / ``f32.head_backward``), forward and backward, against stock fp32.

The stock backward is timed as forward + backward minus the forward of the same window set (autograd has no
backward-only entry point); both figures are in the output.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.adamw_bw import timeit_many  # noqa: E402
from ddpx.ops import f32  # noqa: E402
from ddpx.ops.head import head_backward, head_forward  # noqa: E402

M = 512
CLASSES = (10, 100, 128)


def _report(name, t):
    res = {k: {"us": med, "min_us": lo, "max_us": hi} for k, (med, lo, hi) in t.items()}
    print(name, json.dumps(res), flush=True)
    return res


def _inputs(dev, K, C, dtype):
    g = torch.Generator().manual_seed(C + K)
    h = torch.relu(torch.randn(M, K, generator=g)).to(dtype).to(dev)
    w = (torch.randn(C, K, generator=g) * 0.03).to(dtype).to(dev)
    b = torch.zeros(C, device=dev)
    a = torch.randint(0, C, (M,), generator=g).to(dev)
    return h, w, b, a


def bf16_groups(dev, K, reps, inner):
    fwd, bwd, fused, keep = {}, {}, {}, []
    go = torch.ones((), device=dev)
    lr = torch.full((), 0.1, device=dev)
    for C in CLASSES:
        h, w, b, a = _inputs(dev, K, C, torch.bfloat16)
        _, _, dl = head_forward(h, w, b, a, want_logits=False)
        dW, db, dbp = torch.empty(C, K, device=dev), torch.empty(C, device=dev), torch.empty(K, device=dev)
        dH = torch.empty_like(h)
        params = (w.float(), b, torch.zeros(K, device=dev))  # W, head bias, previous layer's bias
        st = [(x.clone(), torch.zeros_like(x), x.to(torch.bfloat16)) for x in params]
        sgd = [(p, m, s, lr, 0.9, 5e-4) for p, m, s in st]
        hs, ws, bs = h.float().requires_grad_(), w.float().requires_grad_(), b.clone().requires_grad_()

        def stock_fwd(hs=hs, ws=ws, bs=bs, a=a):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return F.cross_entropy(F.linear(hs, ws, bs), a)

        def stock_fb(f=stock_fwd, hs=hs, ws=ws, bs=bs):
            hs.grad = ws.grad = bs.grad = None
            f().backward()
        tag = f"c{C}"
        fwd["native_" + tag] = lambda h=h, w=w, b=b, a=a: head_forward(h, w, b, a, want_logits=False)
        fwd["stock_" + tag] = stock_fwd
        bwd["native_" + tag] = lambda dl=dl, h=h, w=w, dW=dW, db=db, dH=dH, dbp=dbp: head_backward(
            dl, go, h, w, dW, db, dH=dH, dbprev=dbp, relu_mask=True)
        bwd["stock_fwd_" + tag] = stock_fwd
        bwd["stock_fwd_bwd_" + tag] = stock_fb
        # the fused update rewrites the shadow it reads as W: same values class by class, the timing does not care
        fused["native_" + tag] = lambda dl=dl, h=h, sgd=sgd, dH=dH: head_backward(
            dl, go, h, sgd[0][2], None, None, dH=dH, relu_mask=True, sgd_w=sgd[0], sgd_b=sgd[1], sgd_prev=sgd[2])
        keep.append((h, w, b, a, dl, st))
    out = {"fwd": _report(f"bf16_fwd_K{K}", timeit_many(fwd, reps=reps, inner=inner)),
           "bwd_stored": _report(f"bf16_bwd_stored_K{K}", timeit_many(bwd, reps=reps, inner=inner)),
           "bwd_fused_sgd": _report(f"bf16_bwd_fused_sgd_K{K}", timeit_many(fused, reps=reps, inner=inner))}
    for C in CLASSES:
        r = out["bwd_stored"]
        r[f"stock_bwd_c{C}"] = {"us": round(r[f"stock_fwd_bwd_c{C}"]["us"] - r[f"stock_fwd_c{C}"]["us"], 2)}
    return out


def f32_groups(dev, K, reps, inner):
    fwd, bwd, keep = {}, {}, []
    go = torch.ones((), device=dev)
    for C in CLASSES:
        h, w, b, a = _inputs(dev, K, C, torch.float32)
        _, _, dl = f32.head_forward(h, w, b, a)
        dW, db = torch.empty(C, K, device=dev), torch.empty(C, device=dev)
        hs, ws, bs = h.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()

        def stock_fwd(hs=hs, ws=ws, bs=bs, a=a):
            return F.cross_entropy(F.linear(hs, ws, bs), a)

        def stock_fb(f=stock_fwd, hs=hs, ws=ws, bs=bs):
            hs.grad = ws.grad = bs.grad = None
            f().backward()
        tag = f"c{C}"
        fwd["native_" + tag] = lambda h=h, w=w, b=b, a=a: f32.head_forward(h, w, b, a)
        fwd["stock_" + tag] = stock_fwd
        bwd["native_" + tag] = lambda dl=dl, h=h, w=w, dW=dW, db=db: f32.head_backward(dl, go, h, w, dW, db,
                                                                                      relu_mask=True)
        bwd["stock_fwd_" + tag] = stock_fwd
        bwd["stock_fwd_bwd_" + tag] = stock_fb
        keep.append((h, w, b, a, dl))
    out = {"fwd": _report(f"f32_fwd_K{K}", timeit_many(fwd, reps=reps, inner=inner)),
           "bwd": _report(f"f32_bwd_K{K}", timeit_many(bwd, reps=reps, inner=inner))}
    for C in CLASSES:
        r = out["bwd"]
        r[f"stock_bwd_c{C}"] = {"us": round(r[f"stock_fwd_bwd_c{C}"]["us"] - r[f"stock_fwd_c{C}"]["us"], 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda")
    res = {"M": M}
    for K in (512, 4096):
        res[f"bf16_K{K}"] = bf16_groups(dev, K, a.reps, a.inner)
        res[f"f32_K{K}"] = f32_groups(dev, K, a.reps, a.inner)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
