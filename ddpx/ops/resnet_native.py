"""ResNet-9 (``ddpx/models/resnet.py``) as one autograd node on ddpx's MI355X kernels (NHWC, bf16 compute).

The conv -> BatchNorm -> ReLU [-> pool] blocks, the tail and the gradient protocol are VGG's
(``ops/vgg_native.py`` block_forward / block_backward / head_loss / head_grad); what is new is the skip connection,
and it costs no pass of its own:

    forward : the last block of a residual branch adds the skip operand in its BatchNorm apply pass,
              out = res + relu(a*y + b) (``bn_apply(..., res=)``: fp32 add, one rounding);
    backward: with g the gradient at the add's output, the branch runs backwards from g, and the block below
              receives the pair (data gradient of the branch's first convolution, g) in its two-gradient
              BatchNorm backward (``bn_backward(..., gout2=)``): the sum is formed in fp32 inside the kernels and
              never stored.

The data gradient that feeds such a block is the plain ``conv_dgrad``: the BatchNorm-sums epilogue of
``conv_dgrad_bn`` would miss the skip gradient.  Every other block keeps ``conv_dgrad_bn`` as in VGG.  Grad-ready
order is the reverse of the forward (= registration) order, so DDP's buckets, ZeRO-1 and the overlapped optimizer
need nothing new.
"""
from __future__ import annotations

import torch

from . import vgg_native as V
from .vgg_native import _prep_input, plan_of


def _forward(model, x, targets, want_logits, want_grad, training, soft=None):
    plan = plan_of(model)
    flat = model.classifier.weight._ddpx_flat
    saved, outs = [], {}
    for bi in range(len(plan.blocks)):
        k = plan.skip[bi]
        x, sv = V.block_forward(model, plan, flat, bi, x, training, res=None if k is None else outs.pop(k))
        saved.append(sv)
        if bi in plan.skipped:
            outs[bi] = x
    last, loss, logits, dl = V.head_loss(model, flat, x, targets, want_logits, want_grad, soft)
    return saved, last, loss, logits, dl


def _backward(model, saved, last, dl, grad_out):
    plan = plan_of(model)
    flat = model.classifier.weight._ddpx_flat
    g = V.head_grad(model, flat, last, dl, grad_out)
    comm = V._sync_comm(model, True)
    gpart = None
    skip_g = {}  # block index -> the gradient its output receives through the skip connection
    for bi in range(len(plan.blocks) - 1, -1, -1):
        if plan.skip[bi] is not None:  # the add's output gradient goes to the branch and, unchanged, to the skip
            skip_g[plan.skip[bi]] = g
        g, gpart = V.block_backward(model, plan, flat, saved, bi, g, gpart, comm, g2=skip_g.pop(bi, None),
                                    fuse_below=V._BN_BWD_FUSE and (bi - 1) not in plan.skipped)


class _ResNetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, targets, model, soft, *params):
        saved, last, loss, _, dl = _forward(model, x, targets, False, True, model.training, soft)
        ctx.model, ctx.saved, ctx.last, ctx.dl, ctx.n = model, saved, last, dl, len(params)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        _backward(ctx.model, ctx.saved, ctx.last, ctx.dl, grad_loss)
        ctx.saved = ctx.last = ctx.dl = None
        return (None, None, None, None) + (None,) * ctx.n


class _ResNetLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, *params):
        saved, last, _, logits, _ = _forward(model, x, None, True, False, model.training)
        ctx.model, ctx.saved, ctx.last, ctx.n = model, saved, last, len(params)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        _backward(ctx.model, ctx.saved, ctx.last, grad_logits.float().contiguous(), None)
        ctx.saved = ctx.last = None
        return (None, None) + (None,) * ctx.n


def resnet_loss(model, x, targets, soft=None):
    return _ResNetLoss.apply(_prep_input(x), targets, model, soft, *model.parameters())


def resnet_forward(model, x):
    x = _prep_input(x)
    if not torch.is_grad_enabled():
        _, _, _, logits, _ = _forward(model, x, None, True, False, model.training)
        return logits
    return _ResNetLogits.apply(x, model, *model.parameters())
