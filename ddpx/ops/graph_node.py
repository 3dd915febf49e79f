"""The one autograd node pair every native model graph runs under.

A native graph (``vgg_native.py``, ``deepnn_native.py``, ``mlp.py``, ``f32_native.py``) is a forward and a backward
sequence of kernel launches that writes its parameter gradients itself (``FlatParams`` grad protocol) — autograd
only has to call the backward once, when the gradient of the loss (or of the logits) arrives:

    forward(model, x, targets, soft, for_loss) -> (*state, loss, logits, dl)
        ``for_loss``: the fused head returns the loss and its logit gradient ``dl`` (LossNode); otherwise the logits
        alone, with ``targets`` and ``soft`` None (LogitsNode).  ``state``: whatever the backward needs, opaque here.
    backward(model, *state, dl, grad_out)
        ``grad_out``: the gradient of the loss, folded into ``dl`` by the head's backward kernel, or None when ``dl``
        already is the gradient of the logits.

The nodes take the parameters as inputs only so that their output requires grad; every input gets a None gradient.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch


class Graph(NamedTuple):
    forward: Callable
    backward: Callable


class LossNode(torch.autograd.Function):
    """``LossNode.apply(graph, x, targets, model, soft, *params)`` -> the graph's loss."""

    @staticmethod
    def forward(ctx, graph, x, targets, model, soft, *params):
        *state, loss, _, dl = graph.forward(model, x, targets, soft, True)
        ctx.graph, ctx.model, ctx.state, ctx.dl, ctx.n = graph, model, state, dl, len(params)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        ctx.graph.backward(ctx.model, *ctx.state, ctx.dl, grad_loss)
        ctx.state = ctx.dl = None
        return (None,) * (5 + ctx.n)


class LogitsNode(torch.autograd.Function):
    """``LogitsNode.apply(graph, x, model, *params)`` -> the graph's logits."""

    @staticmethod
    def forward(ctx, graph, x, model, *params):
        *state, _, logits, _ = graph.forward(model, x, None, None, False)
        ctx.graph, ctx.model, ctx.state, ctx.n = graph, model, state, len(params)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        ctx.graph.backward(ctx.model, *ctx.state, grad_logits.float().contiguous(), None)
        ctx.state = None
        return (None,) * (3 + ctx.n)
