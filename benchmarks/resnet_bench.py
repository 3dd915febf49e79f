#!/usr/bin/env python3
"""ResNet-9: the skip connection fused into the BatchNorm kernels, and a whole training step.

    python benchmarks/resnet_bench.py [--section kernels|step|join|step18|join_pad|step20|preact_add|step_preact18|conv1x1_s1|all] [--batch 512] [--windows 9] [--out FILE]

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

(c) ``join``: ResNet-18's join kernels (``bn_join`` / ``bn_join_backward``) against their composition from the
    earlier kernels plus torch elementwise ops, at [N,32,32,64] identity, [N,16,16,128] projection, [N,4,4,512] identity.
(d) ``step18``: (b) for ``--model resnet18`` in bf16.
(e) ``join_pad``: the option-A join (``bn_join(pad=)`` / ``bn_join_backward(pad=)``) at [N,16,16,32] and [N,8,8,64]
    against the composition it replaces (torch gather + pad, the identity join, and an identity backward whose skip
    gradient is then zero-inserted by torch ops), and the block below's backward with ``gout2_sub`` against the same
    kernel family with a dense zero-inserted ``gout2``.
(f) ``step20``: (b) for ``--model resnet20`` and ``resnet56`` in bf16.
(g) ``preact_add``: the pre-activation block's kernels at [N,32,32,64], [N,16,16,128] and [N,4,4,512]: ``preact_add``
    + ``bn_finalize`` against a torch add, a torch statistics pass (``var_mean``) and ``bn_finalize`` of its one
    tile; ``bn_backward(gadd=)`` against ``bn_backward`` followed by a torch add.
(h) ``step_preact18``: (b) for ``--model preact_resnet18`` in bf16.
(i) ``conv1x1_s1``: the 1x1 / stride-1 projection kernels (forward, data gradient, weight gradient with its slab
    reduce) at 16 -> 64 and 16 -> 128 on [N,32,32,.] against ``torch.matmul`` on the same bf16 operands and against
    a plain device copy that moves the same number of bytes (half of them read, half written).

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


def join_section(a):
    """ResNet-18's join kernels against their composition from the kernels that came before them plus torch
    elementwise ops.  Forward: relu(bn_apply(y, relu=False) + s), s = res or bn_apply(y2, relu=False).  Backward:
    m = (g + g2) * (out > 0) by torch ops, then one bn_backward of m per BatchNorm, its own ReLU mask held open (b =
    1e30); the composition's dy lacks the factor a, which changes no byte moved."""
    from ddpx.ops import conv as K
    dev = torch.device("cuda")
    N = a.batch
    for (H, C, proj) in ((32, 64, False), (16, 128, True), (4, 512, False)):
        torch.manual_seed(0)
        co = lambda: (torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2,  # noqa: E731
                      torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5)
        av, bv, mean, rstd = co()
        a2, b2, mean2, rstd2 = co()
        y = torch.randn(N * H * H, C, device=dev).to(torch.bfloat16)
        s = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)  # res, or the 1x1 convolution's raw output
        g1 = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        g2 = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        dg, db, dg2, db2 = (torch.empty(C, device=dev) for _ in range(4))
        one, big = torch.ones(C, device=dev), torch.full((C,), 1e30, device=dev)
        if proj:
            fwd = {"fused": lambda: K.bn_join(y, av, bv, N, H, H, C, proj=(s, a2, b2)),
                   "unfused": lambda: torch.relu_(K.bn_apply(y, av, bv, N, H, H, C, relu=False)
                                                  + K.bn_apply(s, a2, b2, N, H, H, C, relu=False))}
        else:
            fwd = {"fused": lambda: K.bn_join(y, av, bv, N, H, H, C, res=s),
                   "unfused": lambda: torch.relu_(K.bn_apply(y, av, bv, N, H, H, C, relu=False) + s)}
        out = fwd["fused"]()

        def unfused_bwd():
            m = (g1 + g2) * (out > 0)
            # y -> (y - mean) * rstd needs the block's own mean / rstd; the open mask comes from a = 1, b = 1e30
            dy = K.bn_backward(m, y, one, big, mean, rstd, N, H, H, C, False, dgamma=dg, dbeta=db)
            if proj:
                return dy, K.bn_backward(m, s, one, big, mean2, rstd2, N, H, H, C, False, dgamma=dg2, dbeta=db2)
            return dy, m

        if proj:
            fused_bwd = lambda: K.bn_join_backward(g1, y, av, bv, mean, rstd, N, H, H, C,  # noqa: E731
                                                   proj=(s, a2, b2, mean2, rstd2), gout2=g2, dgamma=dg, dbeta=db,
                                                   dgamma2=dg2, dbeta2=db2)
        else:
            fused_bwd = lambda: K.bn_join_backward(g1, y, av, bv, mean, rstd, N, H, H, C, res=s, gout2=g2,  # noqa: E731
                                                   dgamma=dg, dbeta=db)
        for which, cands in (("forward", fwd), ("backward", {"fused": fused_bwd, "unfused": unfused_bwd})):
            w = windows(cands, a.windows, a.calls)
            fu, un = stats(w["fused"]), stats(w["unfused"])
            emit(section="join", shape=[N, H, H, C], mode="projection" if proj else "identity", op=which, fused=fu,
                 unfused=un, unfused_spread_pct=round(100 * (un["max_us"] - un["min_us"]) / un["median_us"], 1),
                 fused_over_unfused=round(fu["median_us"] / un["median_us"], 3))


def join_pad_section(a):
    """The option-A join against its composition.  Forward: s = F.pad(x[:, ::2, ::2], ...) by torch ops, then the
    identity join.  Backward: the identity join backward on that s, then the zero insertion of gm's middle channels
    into an array of x's shape (what the block below would read as its dense gout2).  Block below: the identity
    join backward at x's shape with gout2_sub = gs against gout2 = that zero-inserted array (its making not timed)."""
    from ddpx.ops import conv as K
    dev = torch.device("cuda")
    N = a.batch
    bf = torch.bfloat16
    for (Hx, C) in ((32, 32), (16, 64)):
        H, Ch = Hx // 2, C // 2
        torch.manual_seed(0)
        co = lambda n: (torch.rand(n, device=dev) + 0.5, torch.randn(n, device=dev) * 0.2,  # noqa: E731
                        torch.randn(n, device=dev) * 0.1, torch.rand(n, device=dev) + 0.5)
        av, bv, mean, rstd = co(C)
        y, g1, g2 = (torch.randn(N, H, H, C, device=dev).to(bf) for _ in range(3))
        x = torch.randn(N, Hx, Hx, Ch, device=dev).to(bf)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        gather = lambda: F.pad(x[:, ::2, ::2, :], (C // 4, C // 4)).contiguous()  # noqa: E731
        s = gather()

        def unfused_bwd():
            dy, gm = K.bn_join_backward(g1, y, av, bv, mean, rstd, N, H, H, C, res=s, gout2=g2, dgamma=dg, dbeta=db)
            dense = torch.zeros_like(x)
            dense[:, ::2, ::2, :] = gm.view(N, H, H, C)[..., C // 4:3 * C // 4]
            return dy, dense

        cands = {"forward": {"fused": lambda: K.bn_join(y, av, bv, N, H, H, C, pad=x),
                             "unfused": lambda: K.bn_join(y, av, bv, N, H, H, C, res=gather())},
                 "backward": {"fused": lambda: K.bn_join_backward(g1, y, av, bv, mean, rstd, N, H, H, C, pad=x,
                                                                  gout2=g2, dgamma=dg, dbeta=db),
                              "unfused": unfused_bwd}}
        # the block below: identity join at x's shape, second gradient compact or dense
        a1, b1, m1, r1 = co(Ch)
        yb, gb, sb = (torch.randn(N, Hx, Hx, Ch, device=dev).to(bf) for _ in range(3))
        gs = cands["backward"]["fused"]()[1]
        dense = unfused_bwd()[1]
        d1, e1 = torch.empty(Ch, device=dev), torch.empty(Ch, device=dev)
        cands["below"] = {k: (lambda kw=kw: K.bn_join_backward(gb, yb, a1, b1, m1, r1, N, Hx, Hx, Ch, res=sb,
                                                               dgamma=d1, dbeta=e1, **kw))
                          for k, kw in (("fused", dict(gout2_sub=gs)), ("unfused", dict(gout2=dense)))}
        for which, cd in cands.items():
            w = windows(cd, a.windows, a.calls)
            fu, un = stats(w["fused"]), stats(w["unfused"])
            emit(section="join_pad", shape=[N, Hx, Hx, Ch] if which == "below" else [N, H, H, C], op=which, fused=fu,
                 unfused=un, unfused_spread_pct=round(100 * (un["max_us"] - un["min_us"]) / un["median_us"], 1),
                 fused_over_unfused=round(fu["median_us"] / un["median_us"], 3))


def preact_add_section(a):
    """The pre-activation block's two kernels against their compositions.  Forward: z = y + s and the BatchNorm
    coefficients of z.  Backward: the BatchNorm backward with the skip gradient added to its result."""
    from ddpx.ops import conv as K
    dev = torch.device("cuda")
    N = a.batch
    for (H, C) in ((32, 64), (16, 128), (4, 512)):
        torch.manual_seed(0)
        M = N * H * H
        y, s, g, ga = (torch.randn(M, C, device=dev).to(torch.bfloat16) for _ in range(4))
        bn = torch.nn.BatchNorm2d(C).to(dev)
        av, bv, mean, rstd = (torch.empty(C, device=dev) for _ in range(4))
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)

        def fused_fwd():
            z, st, T, BM = K.preact_add(y, s, N, H, H, C)
            K.bn_finalize(st, T, BM, M, bn, True, av, bv, mean, rstd)
            return z

        def unfused_fwd():
            z = y + s
            var, mu = torch.var_mean(z, 0, unbiased=False)
            st = torch.stack([mu.float(), var.float() * M]).view(1, 2, C)
            K.bn_finalize(st, 1, M, M, bn, True, av, bv, mean, rstd)
            return z

        z = fused_fwd()
        bwd = {"fused": lambda: K.bn_backward(g, z, av, bv, mean, rstd, N, H, H, C, False, dgamma=dg, dbeta=db,
                                              gadd=ga),
               "unfused": lambda: K.bn_backward(g, z, av, bv, mean, rstd, N, H, H, C, False, dgamma=dg, dbeta=db) + ga}
        for which, cands in (("forward", {"fused": fused_fwd, "unfused": unfused_fwd}), ("backward", bwd)):
            w = windows(cands, a.windows, a.calls)
            fu, un = stats(w["fused"]), stats(w["unfused"])
            emit(section="preact_add", shape=[N, H, H, C], op=which, fused=fu, unfused=un,
                 unfused_spread_pct=round(100 * (un["max_us"] - un["min_us"]) / un["median_us"], 1),
                 fused_over_unfused=round(fu["median_us"] / un["median_us"], 3))


def conv1x1_s1_section(a):
    """The weight-stationary 1x1 / stride-1 kernels against torch.matmul and a copy of the same bytes."""
    from ddpx.ops import conv as K
    dev = torch.device("cuda")
    N, H, C = a.batch, 32, 16
    P = N * H * H
    for Co in (64, 128):
        torch.manual_seed(0)
        x = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        dy = torch.randn(P, Co, device=dev).to(torch.bfloat16)
        w = torch.randn(Co, C, 1, 1, device=dev) * 0.1
        wf = torch.empty(Co * C, dtype=torch.bfloat16, device=dev)
        K.weight_prep_1x1(w, wf, wf)
        x2, w2 = x.view(P, C), wf.view(Co, C)
        dw = torch.empty(Co * C, device=dev)
        big, small = P * Co * 2, P * C * 2  # bytes of the [P, Co] and the [P, C] operand
        src = torch.empty((big + small) // 4, dtype=torch.bfloat16, device=dev)
        dst = torch.empty_like(src)
        ops = {"forward": (lambda: K.conv1x1_s1_fwd(x, wf, Co), lambda: torch.matmul(x2, w2.t())),
               "dgrad": (lambda: K.conv1x1_s1_dgrad(dy, wf, N, H, H, C, Co), lambda: torch.matmul(dy, w2)),
               "wgrad": (lambda: K.conv1x1_s1_wgrad(dy, x, Co, C, out=dw), lambda: torch.matmul(dy.t(), x2))}
        for which, (native_fn, torch_fn) in ops.items():
            w_ = windows({"native": native_fn, "torch": torch_fn, "copy": lambda: dst.copy_(src)}, a.windows, a.calls)
            na, to, cp = stats(w_["native"]), stats(w_["torch"]), stats(w_["copy"])
            emit(section="conv1x1_s1", shape=[N, H, H, C], Co=Co, op=which, bytes=big + small, native=na,
                 torch_matmul=to, copy_same_bytes=cp,
                 torch_spread_pct=round(100 * (to["max_us"] - to["min_us"]) / to["median_us"], 1),
                 native_over_torch=round(na["median_us"] / to["median_us"], 3),
                 native_over_copy=round(na["median_us"] / cp["median_us"], 3),
                 native_GBps=round((big + small) / na["median_us"] / 1e3, 1))


def step_section(a, name="resnet9", dtypes=("bf16", "fp32")):
    import ddpx
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.models import build_model
    from ddpx.optim import SGD
    from ddpx.train.trainer import Trainer
    dev = torch.device("cuda")
    N = a.batch
    for dtype in dtypes:
        torch.manual_seed(0)
        model = build_model(name, dtype=dtype, device=dev, kernels="native")
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
        stock = build_model(name, dtype=dtype, device=dev, kernels="torch").to(dev)
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
        emit(section="step", model=name, batch=N, dtype=dtype, native_captured=na, stock_eager=st,
             stock_over_native=round(st["median_us"] / na["median_us"], 3), channels_last=bool(a.channels_last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["kernels", "step", "join", "step18", "join_pad", "step20",
                                                         "preact_add", "step_preact18", "conv1x1_s1", "all"])
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
    if a.section in ("join", "all"):
        join_section(a)
    if a.section in ("step18", "all"):
        step_section(a, "resnet18", ("bf16",))
    if a.section in ("join_pad", "all"):
        join_pad_section(a)
    if a.section in ("step20", "all"):
        step_section(a, "resnet20", ("bf16",))
        step_section(a, "resnet56", ("bf16",))
    if a.section in ("preact_add", "all"):
        preact_add_section(a)
    if a.section in ("step_preact18", "all"):
        step_section(a, "preact_resnet18", ("bf16",))
    if a.section in ("conv1x1_s1", "all"):
        conv1x1_s1_section(a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
