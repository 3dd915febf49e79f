#!/usr/bin/env python3
"""What gradient clipping by global norm costs (``--clip_grad_norm``, ``SGD(max_grad_norm=...)``).

Two measurements, JSON to stdout and ``--out``:

``optimizer``  the optimizer stream at the toy MLP's flat size (about 29.4 M elements), fp32 and bf16 gradient
    buffers, HIP events, warm clocks, the variants interleaved inside every repeat of one process:
      sgd        ``sgd_flat_`` over the whole store (the unclipped update)
      clip_sgd   partials + reduce + coef + ``sgd_flat_(clip=...)`` (the clipped update)
      norm       the sum-of-squares pass alone -> achieved read GB/s (gradient bytes / time)
      torch_norm ``torch.linalg.vector_norm`` over the same buffer (a streaming-read reference, same process)
    each with plain and with non-temporal loads in the sum-of-squares pass (``ddpx_grad_sumsq_set_nt``).

``trainer``  whole steps through ``Trainer``: ``singlegpu.py --model mlp --no_fused_optimizer`` against the same
    run plus ``--clip_grad_norm 1e9`` (both take the unfused path, the clip never bites: the difference is the
    price of the feature), alternating fresh child processes, samples/s of the epochs after the first.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_interleaved(variants, reps=15, inner=10, warm=3):
    """{name: median µs per call}: every repeat times each variant once (``inner`` back-to-back calls between
    two events), so clock and neighbour drift hit all variants alike."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) * 1000 / inner)
    return {k: {"us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in ts.items()}


def optimizer_stream(dev):
    import ddpx
    from ddpx.models import MLP
    from ddpx.ops.clip import GradNormPlan
    from ddpx.ops.elementwise import sgd_flat_
    from ddpx.runtime import native
    lib = native.kernels()
    out = {}
    for gd in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        m = MLP()
        ddpx.prepare_model(m, dev, grad_dtype=gd)
        flat = m.fc0.weight._ddpx_flat
        n = flat.total
        flat.grad.copy_((torch.randn(n, device=dev) * 1e-3).to(gd))
        buf = torch.zeros(n, device=dev)
        lr = torch.full((), 1e-3, device=dev)
        plan = GradNormPlan(flat)
        elems = sum(flat.numels)

        def sgd():
            sgd_flat_(flat.master, buf, flat.grad, flat.shadow, lr, 0.9, 5e-4)

        def norm():
            plan.partials(0)

        def clip_sgd():
            plan.partials(0)
            plan.reduce()
            plan.coef(1e9)
            sgd_flat_(flat.master, buf, flat.grad, flat.shadow, lr, 0.9, 5e-4, clip=plan.coef_dev)

        def torch_norm():
            torch.linalg.vector_norm(flat.grad)

        row = {"elements": elems, "flat_total": n, "chunks": plan.n_chunks,
               "grad_bytes": elems * flat.grad.element_size()}
        for nt in (0, 1):
            lib.ddpx_grad_sumsq_set_nt(nt)
            r = _time_interleaved({"sgd": sgd, "clip_sgd": clip_sgd, "norm": norm, "torch_norm": torch_norm})
            r["norm"]["GBps"] = round(row["grad_bytes"] / r["norm"]["us"] / 1e3, 1)
            r["torch_norm"]["GBps"] = round(n * flat.grad.element_size() / r["torch_norm"]["us"] / 1e3, 1)
            r["clip_extra_us"] = round(r["clip_sgd"]["us"] - r["sgd"]["us"], 2)
            row["nt_loads" if nt else "plain_loads"] = r
        lib.ddpx_grad_sumsq_set_nt(0)
        out[str(gd)[6:]] = row
        del m, flat, plan, buf
        torch.cuda.empty_cache()
    return out


def trainer_steps(epochs, rounds, workdir):
    """samples/s of epochs 1.. of ``singlegpu.py`` runs, base and clip alternating as fresh processes."""
    base = [sys.executable, os.path.join(ROOT, "singlegpu.py"), str(epochs), "1000", "--model", "mlp", "--dtype",
            "bf16", "--data", "synthetic", "--no_eval", "--no_fused_optimizer", "--seed", "0"]
    res = {"base": [], "clip": []}
    for r in range(rounds):
        for name, extra in (("base", []), ("clip", ["--clip_grad_norm", "1e9"])):
            mf = os.path.join(workdir, f"{name}{r}.jsonl")
            p = subprocess.run(base + extra + ["--metrics", mf], cwd=workdir, capture_output=True, text=True,
                               timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"{name} run failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            recs = [json.loads(ln) for ln in open(mf) if ln.strip()]
            ep = [x for x in recs if "samples_per_s" in x]
            res[name].append({"samples_per_s": [round(x["samples_per_s"], 1) for x in ep[1:]],
                              "grad_norm": ep[-1].get("grad_norm")})
    for name in ("base", "clip"):
        allv = [v for run in res[name] for v in run["samples_per_s"]]
        res[name + "_median_samples_per_s"] = round(statistics.median(allv), 1)
    b, c = res["base_median_samples_per_s"], res["clip_median_samples_per_s"]
    res["batch_size"] = 512
    res["step_us_base"] = round(512 / b * 1e6, 1)
    res["step_us_clip"] = round(512 / c * 1e6, 1)
    res["clip_extra_us_per_step"] = round(res["step_us_clip"] - res["step_us_base"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_trainer", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs a GPU: a CPU timing says nothing about the MI355X")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "optimizer": optimizer_stream(dev)}
    if not a.skip_trainer:
        with tempfile.TemporaryDirectory() as td:
            res["trainer"] = trainer_steps(a.epochs, a.rounds, td)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
