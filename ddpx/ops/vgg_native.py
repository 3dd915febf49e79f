"""The conv -> BatchNorm -> ReLU networks, VGG (the reference's) and the ResNets of ``ddpx/models/resnet.py``, as one
autograd node on ddpx's MI355X kernels (NHWC, bf16 compute).  The same graphs in fp32: ``ops/f32_native.py``; the
model walk both share: ``ops/plan.py``; the node: ``ops/graph_node.py``.

Per conv block (``/root/reference/singlegpu.py:60-70``):

    forward : y   = conv3x3(x, W)                implicit-GEMM MFMA, epilogue emits BN tile statistics
              a,b = bn_finalize(stats)           Chan merge, running-stat update (momentum 0.1, unbiased var)
              x'  = [maxpool2](relu(a*y + b))    one fused elementwise pass
    backward: dy  = bn_backward(g, y)            pool routing + ReLU mask recomputed from y; dγ, dβ
              dW  = wgrad(dy, x)                 split-K MFMA, fixed-order reduce, torch weight layout
              g   = dgrad(dy, W)                 (skipped for the first block)

then ``x.mean([2,3])`` (global average pool; or the model's scaled global max pool) and the classifier +
cross-entropy on the fused head.

The skip connection of a residual network (``plan.skip``; VGG has none, and the loops then issue the plain calls)
costs no pass of its own:

    forward : the last block of a residual branch adds the skip operand in its BatchNorm apply pass,
              out = res + relu(a*y + b) (``bn_apply(..., res=)``: fp32 add, one rounding);
    backward: with g the gradient at the add's output, the branch runs backwards from g, and the block below
              receives the pair (data gradient of the branch's first convolution, g) in its two-gradient
              BatchNorm backward (``bn_backward(..., gout2=)``): the sum is formed in fp32 inside the kernels and
              never stored.

The data gradient that feeds such a block is the plain ``conv_dgrad``: the BatchNorm-sums epilogue of
``conv_dgrad_bn`` would miss the skip gradient.  Every other block keeps ``conv_dgrad_bn``.  Grad-ready order is the
reverse of the forward (= registration) order, so DDP's buckets, ZeRO-1 and the overlapped optimizer need nothing
for a residual network.

A network of basic residual blocks (ResNet-18, ``plan.stride`` / ``plan.join``) runs on the same loop:

    stride 2: the block's convolution is ``conv_s2_fwd`` / ``conv_s2_dgrad`` / ``conv_s2_wgrad``;
    forward : the second block of a residual block ends in the join, out = relu(a*y + b + s) (``bn_join``), s the
              residual block's input or the BatchNorm of its 1x1 / stride-2 convolution (``conv1x1_s2_fwd``, its
              prepared weight in the plan);
    backward: the join's output receives (g, g2) = (data gradient of the next residual block's first convolution,
              that block's shortcut gradient); ``bn_join_backward`` gives dy for the branch and, for the shortcut,
              gm = bf16((g + g2) * mask) (identity) or dy2, which goes through ``conv1x1_s2_wgrad`` /
              ``conv1x1_s2_dgrad`` (projection).  The shortcut gradient is the second gradient of the block below
              the residual block (a join, or the stem's ``bn_backward(gout2=)``).

The CIFAR ResNet-20/32/44/56 (``plan.PAD``) replace the projection by the parameter-free option-A shortcut:

    forward : the join of a downsampling block takes the block's input, ``bn_join(pad=x)``, and gathers and
              zero-pads the shortcut inside the kernel;
    backward: ``bn_join_backward(pad=x)`` returns the skip gradient compact, gs [N, H, W, C/2]; the join below
              (``plan.sub``) receives (``conv_s2_dgrad`` output, ``gout2_sub=gs``).

``conv_dgrad_bn`` then serves only conv2 -> bn1 inside a residual block; the data gradients that feed a join are the
plain or the strided ones.  Gradients complete in reverse registration order here too (``models/resnet.py``).

A pre-activation network (``PreActResNet``, ``plan.add``) is the same chain of units with an add between a block's
second convolution and the BatchNorm that reads it:

    forward : ``conv_fwd(stats=False)`` -> z = y + s and the tile statistics of z in one pass (``preact_add``, z in
              y's storage) -> ``bn_finalize`` -> ``bn_apply``; evaluation: ``bn_finalize`` first, then ``preact_add``
              writes z and relu(a*z + b) together.  s is the z of the unit two below (identity) or the raw output of
              ``conv1x1_s2_fwd(stats=False)`` on that unit's output (projection);
    backward: dz, the BatchNorm backward's result, is the output gradient of the unit's convolution and also goes
              down the shortcut: as ``bn_backward(gadd=dz)`` of the unit two below (identity: added on the output
              side of that BatchNorm backward, whose sums may still come from ``conv_dgrad_bn``), or through
              ``conv1x1_s2_wgrad`` / ``conv1x1_s2_dgrad`` as that unit's ``gout2`` (projection).  No copy, no add pass.

``model.sync_bn_comm`` (native SyncBatchNorm, ``--sync_bn``; reference: the commented-out
``convert_sync_batchnorm`` at ``/root/reference/multigpu.py:127``) merges the BatchNorm statistics across
ranks: an all-gather of each rank's [2][C] (mean, M2) in the forward, an all-reduce of (Σdy, Σdy·x̂) in the
backward, both on the compute stream between the same native kernels.
Weight gradients land straight in the DDP bucket storage (grad-ready order: classifier, bn7, conv7,
..., as torch DDP's rebuilt buckets) or — single process with ``SGD(fused_backward=True)`` — are
applied in the reduce kernels without ever being stored.  The forward reads bf16 copies of the conv
weights permuted for the GEMMs (``Wf``: [Co][3][3][Ci], ``Wd``: [3][3][Co][Ci]) that are refreshed from
the fp32 masters once per forward; dgrad reads them, so the fused update of W never races dgrad.
"""
from __future__ import annotations

import os

import torch

from . import conv as K
from ..models.resnet import tail_of
from ..optim.sgd import take_lr_advance
from .graph_node import Graph, LogitsNode, LossNode
from .head import head_backward, head_forward
from .plan import PAD, _sync_comm, conv_adds, conv_blocks, conv_joins
from .plan import plan_of as _plan_of


# DDPX_CONV_PREP_FROM_UPDATE=0: re-derive the bf16 conv layouts every forward (weight_prep) even when the fused
# update already wrote them (A/B checks)
_PREP_FROM_UPDATE = os.environ.get("DDPX_CONV_PREP_FROM_UPDATE", "1") != "0"
# DDPX_BN_BWD_FUSE=0: the BatchNorm backward sums by their own reduce pass over g and y, instead of in the epilogue
# of the conv data gradient that produces g (csrc/include/ddpx_pipe.h EPI_BNBWD_BF16)
_BN_BWD_FUSE = os.environ.get("DDPX_BN_BWD_FUSE", "1") != "0"


class _Plan:
    """Static description of the network + persistent prepared-weight buffers."""

    def __init__(self, model):
        self.blocks, self.skip = conv_blocks(model)
        self.stride, self.join = conv_joins(model)
        self.add = conv_adds(model)  # the shortcut adds of a pre-activation network
        # blocks whose output also feeds a skip connection or the shortcut of a join: their BatchNorm backward
        # receives two gradients
        self.skipped = ({k for k in self.skip if k is not None} | {j[0] for j in self.join if j is not None}
                        | {ad[0] for ad in self.add if ad is not None and ad[1] is not None})
        # blocks whose second gradient comes compact, at the even pixels only: the input of an option-A block
        self.sub = {j[0] for j in self.join if j is not None and j[1] is PAD}
        assert all(self.join[k] is not None for k in self.sub), "an option-A block sits on a join"
        dev = model.classifier.weight.device
        # projection shortcuts: the 1x1 weight as bf16 [Co][Ci], one array for the forward and the data gradient,
        # refreshed on the same version check as the 3x3 layouts
        self.sc_w, self.sc_ver = {}, {}
        for bi, j in enumerate(self.join):
            if j is not None and j[1] is not None and j[1] is not PAD:
                Co, Ci = j[1].weight.shape[:2]
                self.sc_w[bi] = torch.empty(Co * K.padded_channels(Ci), dtype=torch.bfloat16, device=dev)
                self.sc_ver[bi] = None
        for bi, ad in enumerate(self.add):
            if ad is not None and ad[1] is not None:
                Co, Ci = ad[1].weight.shape[:2]
                self.sc_w[bi] = torch.empty(Co * K.padded_channels(Ci), dtype=torch.bfloat16, device=dev)
                self.sc_ver[bi] = None
        self.wf, self.wd = [], []
        for conv, _, _ in self.blocks:
            Co, Ci = conv.weight.shape[:2]
            n = Co * 9 * K.padded_channels(Ci)
            self.wf.append(torch.empty(n, dtype=torch.bfloat16, device=dev))
            self.wd.append(torch.empty(n, dtype=torch.bfloat16, device=dev))
        # FlatParams version of each conv weight the prepared layouts were made from (None: never): the fused
        # single-process update rewrites them in its reduce kernel, any other update makes them stale
        self.wver = [None] * len(self.blocks)


def plan_of(model):
    return _plan_of(model, "_ddpx_plan", _Plan)


def _coefs(Co, dev):
    a = torch.empty(Co, dtype=torch.float32, device=dev)
    return a, torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)


def join_forward(plan, flat, bi, y, a, b, N, H, W, Co, src, training):
    """The BatchNorm apply of the last block of a basic residual block, relu(a*y + b + s), in the join kernel:
    (output, (src, shortcut state)).  ``src``: the residual block's input; s = src (identity), or the BatchNorm of
    its 1x1 / stride-2 convolution (projection), whose raw output and coefficients are the shortcut state, or the
    option-A shortcut gathered from src inside the kernel (``plan.PAD``)."""
    _, sc_conv, sc_bn = plan.join[bi]
    if sc_conv is None:
        return K.bn_join(y, a, b, N, H, W, Co, res=src), (src, None)
    if sc_conv is PAD:
        return K.bn_join(y, a, b, N, H, W, Co, pad=src), (src, None)
    ver = flat.version_of(sc_conv.weight)
    if plan.sc_ver[bi] != ver:
        K.weight_prep_1x1(sc_conv.weight, plan.sc_w[bi], plan.sc_w[bi])
        plan.sc_ver[bi] = ver
    y2, st, T, BM = K.conv1x1_s2_fwd(src, plan.sc_w[bi], Co, stats=training)
    a2, b2, mean2, rstd2 = _coefs(Co, y.device)
    K.bn_finalize(st, T, BM, N * H * W, sc_bn, training, a2, b2, mean2, rstd2)
    return K.bn_join(y, a, b, N, H, W, Co, proj=(y2, a2, b2)), (src, (y2, a2, b2, mean2, rstd2))


def add_forward(plan, flat, bi, y, bn, src, N, H, W, Co, training):
    """The shortcut add of a pre-activation block between convolution ``bi`` and its BatchNorm: z = y + s in y's
    storage.  ``src``: the z of block k (identity) or block k's output, the input of the 1x1 / stride-2 projection
    whose raw output is s.  Training: (z, statistics of z, coefficients, None).  Evaluation: the coefficients come
    first and the same pass also applies them, (z, None, coefficients, relu(a*z + b))."""
    sc_conv = plan.add[bi][1]
    s = src
    if sc_conv is not None:
        ver = flat.version_of(sc_conv.weight)
        if plan.sc_ver[bi] != ver:
            K.weight_prep_1x1(sc_conv.weight, plan.sc_w[bi], plan.sc_w[bi])
            plan.sc_ver[bi] = ver
        s = K.conv1x1_s2_fwd(src, plan.sc_w[bi], Co, stats=False)[0]
    co = _coefs(Co, y.device)
    if training:
        z, st, T, BM = K.preact_add(y, s, N, H, W, Co, out=y)
        return z, (st, T, BM), co, None
    K.bn_finalize(None, 0, 0, N * H * W, bn, False, *co)
    z, act = K.preact_add(y, s, N, H, W, Co, stats=False, out=y, eval_ab=co[:2])
    return z, None, co, act


def block_forward(model, plan, flat, bi, x, training, res=None, src=None):
    """One conv -> BatchNorm -> ReLU [-> pool] block: (output, what its backward needs).  ``res``: the skip operand
    added to the output in the BatchNorm apply pass (the last block of a residual branch).  ``src``: the input of the
    basic residual block that this block ends (``plan.join``): its apply pass is the join; or the shortcut source of
    a pre-activation block's add (``plan.add``, :func:`add_forward`).  (N, H, W) of the saved shape are the block's
    output's (those of x but for a stride-2 convolution)."""
    conv, bn, pool = plan.blocks[bi]
    N, H, W, C = x.shape
    Co = conv.weight.shape[0]
    ver = flat.version_of(conv.weight)
    if plan.wver[bi] != ver:
        K.weight_prep(conv.weight, plan.wf[bi], plan.wd[bi])
        plan.wver[bi] = ver
    add = plan.add[bi] is not None
    if plan.stride[bi] == 2:
        y, st, T, BM = K.conv_s2_fwd(x, plan.wf[bi], Co, stats=training)
        H, W = K.s2_out_hw(H, W)
    else:
        y, st, T, BM = K.conv_fwd(x, plan.wf[bi], Co, stats=training and not add)
    comm = _sync_comm(model, training)
    if add:
        if comm is not None:
            raise RuntimeError("native SyncBatchNorm does not cover the pre-activation add (preact_resnet)")
        y, stt, (a, b, mean, rstd), xn = add_forward(plan, flat, bi, y, bn, src, N, H, W, Co, training)
        if training:
            K.bn_finalize(*stt, N * H * W, bn, True, a, b, mean, rstd)
            xn = K.bn_apply(y, a, b, N, H, W, Co, relu=True, pool=pool)
        return xn, (x, y, a, b, mean, rstd, (N, H, W, C, Co), pool)
    a, b, mean, rstd = _coefs(Co, x.device)
    if comm is not None:
        if any(j is not None for j in plan.join):
            raise RuntimeError("native SyncBatchNorm does not cover the join kernels (resnet18)")
        K.bn_finalize_sync(st, T, BM, N * H * W, bn, a, b, mean, rstd, comm)
    else:
        K.bn_finalize(st, T, BM, N * H * W, bn, training, a, b, mean, rstd)
    sv = (x, y, a, b, mean, rstd, (N, H, W, C, Co), pool)
    if plan.join[bi] is not None:
        xn, jsv = join_forward(plan, flat, bi, y, a, b, N, H, W, Co, src, training)
        return xn, sv + (jsv,)
    xn = K.bn_apply(y, a, b, N, H, W, Co, relu=True, pool=pool, res=res)
    return xn, sv


def head_loss(model, flat, x, targets, want_logits, want_grad, soft=None):
    """Global average pool (or the model's scaled global max pool, ``model.tail == "max"``) + classifier +
    cross-entropy on the fused head: (last, loss, logits, dlogits)."""
    tail, scale = tail_of(model)
    if tail == "max":
        feat = K.gmaxpool(x, scale)
        last = (x, feat)  # the backward recomputes the argmax from the last block's output
    else:
        feat = K.avgpool(x)  # [N, 512] bf16
        last = (x.shape, feat)
    cls = model.classifier
    loss, logits, dl = head_forward(feat, flat.shadow_of(cls.weight), cls.bias, targets, want_logits=want_logits,
                                    want_grad=want_grad, lr_advance=take_lr_advance(flat) if want_grad else None,
                                    soft=soft)
    return last, loss, logits, dl


def _forward(model, x, targets, want_logits, want_grad, training, soft=None):
    plan = plan_of(model)
    flat = model.classifier.weight._ddpx_flat
    saved, outs = [], {}  # outs: the outputs that a later block's skip connection adds, until it has
    for bi in range(len(plan.blocks)):
        k, j, ad = plan.skip[bi], plan.join[bi], plan.add[bi]
        src = None if j is None else outs.pop(j[0])
        if ad is not None:  # identity: block k's pre-BatchNorm sum; projection: its output
            src = saved[ad[0]][1] if ad[1] is None else outs.pop(ad[0])
        x, sv = block_forward(model, plan, flat, bi, x, training, res=None if k is None else outs.pop(k), src=src)
        saved.append(sv)
        if bi in plan.skipped:
            outs[bi] = x
    last, loss, logits, dl = head_loss(model, flat, x, targets, want_logits, want_grad, soft)
    return saved, last, loss, logits, dl


def head_grad(model, flat, last, dl, grad_out):
    """Classifier gradients (stored or applied) and the gradient at the last block's output."""
    cls = model.classifier
    xlast, feat = last
    dfeat = torch.empty_like(feat)
    sw, sb = flat.fused_spec(cls.weight), flat.fused_spec(cls.bias)
    if sw is not None:
        head_backward(dl, grad_out, feat, flat.shadow_of(cls.weight), None, None, dH=dfeat, relu_mask=False,
                      sgd_w=sw, sgd_b=sb)
        flat.mark_updated(cls.weight)
        flat.mark_updated(cls.bias)
    else:
        dW, acc = flat.grad_target(cls.weight)
        db, _ = flat.grad_target(cls.bias)
        head_backward(dl, grad_out, feat, flat.shadow_of(cls.weight), dW, db, dH=dfeat, relu_mask=False,
                      accumulate=acc)
        flat.grad_done(cls.weight)
        flat.grad_done(cls.bias)
    tail, scale = tail_of(model)
    if tail == "max":
        return K.gmaxpool_backward(dfeat, xlast, scale)
    return K.avgpool_backward(dfeat, *xlast)


def _bn_targets(flat, bn, sfx=""):
    """Where a BatchNorm's dgamma / dbeta go, as the keyword arguments of ``K.bn_join_backward`` (``sfx`` "2": the
    shortcut's): the fused SGD specs, or the gradient buffers and whether to accumulate."""
    sg, sb = flat.fused_spec(bn.weight), flat.fused_spec(bn.bias)
    if sg is not None:
        return {"sgd_gamma" + sfx: sg, "sgd_beta" + sfx: sb}
    dgam, acc = flat.grad_target(bn.weight)
    dbet, _ = flat.grad_target(bn.bias)
    return {"dgamma" + sfx: dgam, "dbeta" + sfx: dbet, "accumulate" + sfx: acc}


def _bn_done(flat, bn, targets):
    done = flat.mark_updated if any(k.startswith("sgd") for k in targets) else flat.grad_done
    done(bn.weight)
    done(bn.bias)


def join_backward(plan, flat, saved, bi, g, g2, skip_g):
    """BatchNorm backward of a join block given the gradients (g, g2) of the join's output: dy of the branch's second
    convolution.  The gradient that the shortcut carries to the residual block's input goes to ``skip_g[k]``: gm =
    bf16((g + g2) * mask) for an identity shortcut; for a projection, the data gradient of the 1x1 convolution, whose
    weight gradient and whose BatchNorm's are stored or applied here.  Order of completion: sc_bn, bn, sc_conv.
    An option-A shortcut hands down the compact gs [N, H, W, C/2]; the block below it (``plan.sub``) gets its g2 in
    that form and passes it as ``gout2_sub``."""
    _, bn, _ = plan.blocks[bi]
    _, y, a, b, mean, rstd, (N, H, W, _, Co), _, (src, sc) = saved[bi]
    k, sc_conv, sc_bn = plan.join[bi]
    tg = _bn_targets(flat, bn)
    if sc_conv is None and bi not in plan.sub:
        dy, gm = K.bn_join_backward(g, y, a, b, mean, rstd, N, H, W, Co, res=src, gout2=g2, **tg)
        _bn_done(flat, bn, tg)
        skip_g[k] = gm.view(src.shape)
        return dy
    if sc_conv is None or sc_conv is PAD:
        g2kw = {"gout2_sub": g2} if bi in plan.sub else {"gout2": g2}
        skw = {"res": src} if sc_conv is None else {"pad": src}
        dy, gm = K.bn_join_backward(g, y, a, b, mean, rstd, N, H, W, Co, **skw, **g2kw, **tg)
        _bn_done(flat, bn, tg)
        skip_g[k] = gm.view(src.shape) if sc_conv is None else gm
        return dy
    tg2 = _bn_targets(flat, sc_bn, "2")
    dy, dy2 = K.bn_join_backward(g, y, a, b, mean, rstd, N, H, W, Co, proj=sc, gout2=g2, **tg, **tg2)
    _bn_done(flat, sc_bn, tg2)
    _bn_done(flat, bn, tg)
    w = sc_conv.weight
    sw = flat.fused_spec(w)
    if sw is not None:
        K.conv1x1_s2_wgrad(dy2, src, Co, w.shape[1], sgd=sw)
        flat.mark_updated(w)
    else:
        dw, accw = flat.grad_target(w)
        K.conv1x1_s2_wgrad(dy2, src, Co, w.shape[1], out=dw, accumulate=accw)
        flat.grad_done(w)
    # (the prepared bf16 copy the forward made: a fused update above changed the fp32 master only)
    skip_g[k] = K.conv1x1_s2_dgrad(dy2, plan.sc_w[bi], *src.shape, Co)
    return dy


def add_backward(plan, flat, saved, bi, dz, skip_g, add_g):
    """The shortcut of a pre-activation block, given dz, the gradient at the add between convolution ``bi`` and its
    BatchNorm.  Identity: dz itself is what block k's BatchNorm backward adds on its output side (``add_g[k]``).
    Projection: the 1x1 convolution's weight gradient is stored or applied, and its data gradient is the second
    gradient of block k's output (``skip_g[k]``)."""
    k, sc_conv = plan.add[bi]
    if sc_conv is None:
        add_g[k] = dz
        return
    src = saved[k + 1][0]  # block k's output: the input of block k + 1 (the branch's strided convolution)
    Co, w = saved[bi][6][4], sc_conv.weight
    sw = flat.fused_spec(w)
    if sw is not None:
        K.conv1x1_s2_wgrad(dz, src, Co, w.shape[1], sgd=sw)
        flat.mark_updated(w)
    else:
        dw, accw = flat.grad_target(w)
        K.conv1x1_s2_wgrad(dz, src, Co, w.shape[1], out=dw, accumulate=accw)
        flat.grad_done(w)
    skip_g[k] = K.conv1x1_s2_dgrad(dz, plan.sc_w[bi], *src.shape, Co)


def block_backward(model, plan, flat, saved, bi, g, gpart, comm, g2=None, skip_g=None, gadd=None, add_g=None):
    """Backward of block ``bi`` given the gradient ``g`` of its output (``gpart``: its BatchNorm pass-1 sums, when the
    data gradient that made g produced them; ``g2``: a second gradient of the same output, from a skip connection;
    ``gadd``: the gradient an identity pre-activation shortcut adds on the output side of the BatchNorm backward):
    the parameter gradients stored or applied, and (g, gpart) of the block below (None, None for the first block).
    A join block also leaves the gradient of its shortcut in ``skip_g`` (:func:`join_backward`), a pre-activation add
    in ``skip_g`` or ``add_g`` (:func:`add_backward`)."""
    conv, bn, pool = plan.blocks[bi]
    x, y, a, b, mean, rstd, (N, H, W, C, Co), _ = saved[bi][:8]
    stride = plan.stride[bi]
    # the data gradient may put the BatchNorm backward sums of the block below into its epilogue: not when that
    # block receives a second gradient, which the epilogue would miss (nor has the strided data gradient one)
    fuse_below = _BN_BWD_FUSE and (bi - 1) not in plan.skipped and stride == 1
    sg, sbeta = flat.fused_spec(bn.weight), flat.fused_spec(bn.bias)
    if plan.join[bi] is not None:
        dy = join_backward(plan, flat, saved, bi, g, g2, skip_g)
    elif comm is not None:
        if sg is not None:
            raise RuntimeError("SyncBatchNorm runs under DDP; the fused single-process optimizer does not apply")
        dgam, accg = flat.grad_target(bn.weight)
        dbet, _ = flat.grad_target(bn.bias)
        dy = K.bn_backward_sync(g, y, a, b, mean, rstd, N, H, W, Co, pool, comm, dgamma=dgam, dbeta=dbet,
                                accumulate=accg, part=gpart, gout2=g2)
        flat.grad_done(bn.weight)
        flat.grad_done(bn.bias)
    elif sg is not None:
        dy = K.bn_backward(g, y, a, b, mean, rstd, N, H, W, Co, pool, sgd_gamma=sg, sgd_beta=sbeta, part=gpart,
                           gout2=g2, gadd=gadd)
        flat.mark_updated(bn.weight)
        flat.mark_updated(bn.bias)
    else:
        dgam, accg = flat.grad_target(bn.weight)
        dbet, _ = flat.grad_target(bn.bias)
        dy = K.bn_backward(g, y, a, b, mean, rstd, N, H, W, Co, pool, dgamma=dgam, dbeta=dbet, accumulate=accg,
                           part=gpart, gout2=g2, gadd=gadd)
        flat.grad_done(bn.weight)
        flat.grad_done(bn.bias)
    if plan.add[bi] is not None:
        add_backward(plan, flat, saved, bi, dy, skip_g, add_g)

    def dgrad():
        """g of the block below, with its BatchNorm backward sums from the GEMM epilogue when possible."""
        if stride == 2:
            return K.conv_s2_dgrad(dy, plan.wd[bi], *x.shape, Co), None
        if fuse_below:
            _, yp, ap, bp, mp, rp, _, poolp = saved[bi - 1][:8]
            return K.conv_dgrad_bn(dy, plan.wd[bi], N, H, W, C, Co, yp, ap, bp, mp, rp, poolp)
        return K.conv_dgrad(dy, plan.wd[bi], N, H, W, C, Co), None

    below = (None, None)
    Cr = conv.weight.shape[1]
    sw = flat.fused_spec(conv.weight)
    if sw is not None and stride == 2:  # (the strided reduce writes no prepared layouts: the next forward does)
        K.conv_s2_wgrad(dy, x, Co, Cr, sgd=sw)
        flat.mark_updated(conv.weight)
    elif sw is not None:
        # prepared layouts current before this update (the forward made or kept them): the reduce rewrites
        # them with the updated weight, after this block's dgrad below has read wd (stream order)
        prep = _PREP_FROM_UPDATE and plan.wver[bi] == flat.version_of(conv.weight)
        if prep and bi > 0:
            below = dgrad()
        K.conv_wgrad(dy, x, Co, Cr, sgd=sw, prepared=(plan.wf[bi], plan.wd[bi]) if prep else None)
        flat.mark_updated(conv.weight)
        if prep:
            plan.wver[bi] = flat.version_of(conv.weight)
            return below
    else:
        dw, accw = flat.grad_target(conv.weight)
        (K.conv_s2_wgrad if stride == 2 else K.conv_wgrad)(dy, x, Co, Cr, out=dw, accumulate=accw)
        flat.grad_done(conv.weight)
    if bi > 0:
        below = dgrad()
    return below


def _backward(model, saved, last, dl, grad_out):
    plan = plan_of(model)
    flat = model.classifier.weight._ddpx_flat
    g = head_grad(model, flat, last, dl, grad_out)
    comm = _sync_comm(model, True)
    gpart = None  # BatchNorm pass-1 sums of g, when the data gradient that made g produced them
    skip_g = {}  # block index -> the gradient its output receives through the skip connection
    add_g = {}  # block index -> the gradient its pre-BatchNorm sum receives through an identity pre-activation shortcut
    for bi in range(len(plan.blocks) - 1, -1, -1):
        if plan.skip[bi] is not None:  # the add's output gradient goes to the branch and, unchanged, to the skip
            skip_g[plan.skip[bi]] = g
        g, gpart = block_backward(model, plan, flat, saved, bi, g, gpart, comm, g2=skip_g.pop(bi, None),
                                  skip_g=skip_g, gadd=add_g.pop(bi, None), add_g=add_g)


GRAPH = Graph(lambda model, x, targets, soft, for_loss:
              _forward(model, x, targets, not for_loss, for_loss, model.training, soft), _backward)


def _prep_input(x):
    if x.dim() == 4 and x.shape[-1] == 8 and x.dtype == torch.bfloat16:
        return x.contiguous()
    if x.dim() == 4 and x.shape[1] == 3:  # NCHW fp32 from a reference-style loader
        x = x.permute(0, 2, 3, 1)
        x = torch.nn.functional.pad(x, (0, 8 - x.shape[-1]))
        return x.to(torch.bfloat16).contiguous()
    raise ValueError(f"unsupported VGG input {tuple(x.shape)} {x.dtype}")


def vgg_loss(model, x, targets, soft=None):
    return LossNode.apply(GRAPH, _prep_input(x), targets, model, soft, *model.parameters())


def vgg_forward(model, x):
    x = _prep_input(x)
    if not torch.is_grad_enabled():
        _, _, _, logits, _ = _forward(model, x, None, True, False, model.training)
        return logits
    return LogitsNode.apply(GRAPH, x, model, *model.parameters())
