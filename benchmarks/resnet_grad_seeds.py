#!/usr/bin/env python3
"""fp32 ResNet-9 gradient error vs fp64 over several seeds: the native fp32 path and torch's own fp32 run.

    python benchmarks/resnet_grad_seeds.py [--seeds 8] [--batch 32] [--tail avg|max] [--tail_scale X] [--out FILE]

Below a 2x2 max-pool a gradient moves whenever a window routes to another element because two candidates lie
within fp32 round-off, so one batch says little; this runs the single-batch check of
tests/test_gpu_resnet.py::test_resnet_native_fp32_matches_fp64 on several seeds and reports, per path, the largest
relative error over the parameters below a pooling decision (everything but the classifier).  The test's absolute
cap is 1.5x the largest error torch's own run shows here.  ``--tail max --tail_scale 0.125`` measures the published
tail (tests/test_gpu_resnet_tail.py's cap, profiles/r21_tail/grad_seeds.txt): its 4x4 window adds routing flips.
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tail", default="avg", choices=["avg", "max"])
    ap.add_argument("--tail_scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ddpx
    from ddpx.models import build_model
    gpu = torch.device("cuda")
    rows, lines = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for seed in range(a.seeds):
        torch.manual_seed(seed)
        base = build_model("resnet9", dtype="fp32", device=gpu, kernels="native", tail=a.tail,
                           tail_scale=a.tail_scale)
        x = torch.rand(a.batch, 3, 32, 32, device=gpu)
        y = torch.randint(0, 10, (a.batch,), device=gpu)
        r64 = copy.deepcopy(base).cpu().double()
        r64.use_native = False
        F.cross_entropy(r64(x.cpu().double()), y.cpu()).backward()
        p64 = dict(r64.named_parameters())
        ref = copy.deepcopy(base).to(gpu)
        ref.use_native = False
        F.cross_entropy(ref(x), y).backward()
        errs = {"torch": {n: rel(p.grad.cpu(), p64[n].grad) for n, p in ref.named_parameters()}}
        m = copy.deepcopy(base)
        flat = ddpx.prepare_model(m, gpu)
        flat.zero_grad()
        loss, _ = m.forward_loss(x, y)
        loss.backward()
        errs["native"] = {n: rel(p.main_grad.cpu(), p64[n].grad) for n, p in m.named_parameters()}
        below = [n for n in errs["torch"] if not n.startswith("classifier")]
        row = {"seed": seed, "batch": a.batch, "tail": a.tail, "tail_scale": a.tail_scale,
               **{k: round(max(v[n] for n in below), 7) for k, v in errs.items()},
               **{k + "_classifier": round(max(v[n] for n in v if n.startswith("classifier")), 9)
                  for k, v in errs.items()}}
        rows.append(row)
        say(json.dumps(row))
    for k in ("torch", "native"):
        v = sorted(r[k] for r in rows)
        say(f"{k:7s} max-below-pool error over {len(v)} seeds: median {v[len(v) // 2]:.3e}  max {v[-1]:.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
