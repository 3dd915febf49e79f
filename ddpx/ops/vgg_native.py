"""The conv -> BatchNorm -> ReLU networks, VGG (the reference's) and ResNet-9 (``ddpx/models/resnet.py``), as one
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
from .plan import _sync_comm, conv_blocks
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
        # blocks whose output also feeds a skip connection: their BatchNorm backward receives two gradients
        self.skipped = {k for k in self.skip if k is not None}
        dev = model.classifier.weight.device
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


def block_forward(model, plan, flat, bi, x, training, res=None):
    """One conv -> BatchNorm -> ReLU [-> pool] block: (output, what its backward needs).  ``res``: the skip operand
    added to the output in the BatchNorm apply pass (the last block of a residual branch)."""
    conv, bn, pool = plan.blocks[bi]
    N, H, W, C = x.shape
    Co = conv.weight.shape[0]
    ver = flat.version_of(conv.weight)
    if plan.wver[bi] != ver:
        K.weight_prep(conv.weight, plan.wf[bi], plan.wd[bi])
        plan.wver[bi] = ver
    y, st, T, BM = K.conv_fwd(x, plan.wf[bi], Co, stats=training)
    dev = x.device
    a = torch.empty(Co, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    mean = torch.empty_like(a)
    rstd = torch.empty_like(a)
    comm = _sync_comm(model, training)
    if comm is not None:
        K.bn_finalize_sync(st, T, BM, N * H * W, bn, a, b, mean, rstd, comm)
    else:
        K.bn_finalize(st, T, BM, N * H * W, bn, training, a, b, mean, rstd)
    xn = K.bn_apply(y, a, b, N, H, W, Co, relu=True, pool=pool, res=res)
    return xn, (x, y, a, b, mean, rstd, (N, H, W, C, Co), pool)


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
        k = plan.skip[bi]
        x, sv = block_forward(model, plan, flat, bi, x, training, res=None if k is None else outs.pop(k))
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


def block_backward(model, plan, flat, saved, bi, g, gpart, comm, g2=None):
    """Backward of block ``bi`` given the gradient ``g`` of its output (``gpart``: its BatchNorm pass-1 sums, when the
    data gradient that made g produced them; ``g2``: a second gradient of the same output, from a skip connection):
    the parameter gradients stored or applied, and (g, gpart) of the block below (None, None for the first block)."""
    conv, bn, pool = plan.blocks[bi]
    x, y, a, b, mean, rstd, (N, H, W, C, Co), _ = saved[bi]
    # the data gradient may put the BatchNorm backward sums of the block below into its epilogue: not when that
    # block receives a second gradient, which the epilogue would miss
    fuse_below = _BN_BWD_FUSE and (bi - 1) not in plan.skipped
    sg, sbeta = flat.fused_spec(bn.weight), flat.fused_spec(bn.bias)
    if comm is not None:
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
                           gout2=g2)
        flat.mark_updated(bn.weight)
        flat.mark_updated(bn.bias)
    else:
        dgam, accg = flat.grad_target(bn.weight)
        dbet, _ = flat.grad_target(bn.bias)
        dy = K.bn_backward(g, y, a, b, mean, rstd, N, H, W, Co, pool, dgamma=dgam, dbeta=dbet, accumulate=accg,
                           part=gpart, gout2=g2)
        flat.grad_done(bn.weight)
        flat.grad_done(bn.bias)

    def dgrad():
        """g of the block below, with its BatchNorm backward sums from the GEMM epilogue when possible."""
        if fuse_below:
            _, yp, ap, bp, mp, rp, _, poolp = saved[bi - 1]
            return K.conv_dgrad_bn(dy, plan.wd[bi], N, H, W, C, Co, yp, ap, bp, mp, rp, poolp)
        return K.conv_dgrad(dy, plan.wd[bi], N, H, W, C, Co), None

    below = (None, None)
    Cr = conv.weight.shape[1]
    sw = flat.fused_spec(conv.weight)
    if sw is not None:
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
        K.conv_wgrad(dy, x, Co, Cr, out=dw, accumulate=accw)
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
    for bi in range(len(plan.blocks) - 1, -1, -1):
        if plan.skip[bi] is not None:  # the add's output gradient goes to the branch and, unchanged, to the skip
            skip_g[plan.skip[bi]] = g
        g, gpart = block_backward(model, plan, flat, saved, bi, g, gpart, comm, g2=skip_g.pop(bi, None))


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
