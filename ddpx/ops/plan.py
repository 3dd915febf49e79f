"""What the native model graphs of both precisions read off a model: the walk of each network family into blocks,
the per-model plan cache, the SyncBatchNorm communicator and DeepNN's constant vectors and dropout state.

The graphs themselves: ``vgg_native.py`` (VGG and ResNet-9, bf16), ``deepnn_native.py`` (bf16), ``mlp.py`` (bf16 /
MX-FP8) and ``f32_native.py`` (all of them in fp32).
"""
from __future__ import annotations

import torch
from torch import nn


def conv_blocks(model):
    """(blocks, skip) of a conv -> BatchNorm -> ReLU [-> pool] network: ``blocks[bi] = (conv, bn, pool)`` in forward
    order, ``skip[bi]`` = index of the block whose output is added to block bi's (the end of a residual branch), or
    None.  Residual networks describe themselves (``native_blocks()``, models/resnet.py); VGG is walked from its
    ``backbone``."""
    if hasattr(model, "native_blocks"):
        nb = model.native_blocks()
        return [tuple(b[:3]) for b in nb], [b[3] for b in nb]
    mods = list(model.backbone.children())
    blocks, i = [], 0
    while i < len(mods):
        conv, bn = mods[i], mods[i + 1]
        assert isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)
        i += 3  # conv, bn, relu
        pool = i < len(mods) and isinstance(mods[i], nn.MaxPool2d)
        if pool:
            i += 1
        blocks.append((conv, bn, pool))
    return blocks, [None] * len(blocks)


# join[bi][1] of a parameter-free option-A shortcut (the CIFAR ResNet-20/32/44/56), in place of sc_conv
PAD = "pad"


def conv_joins(model):
    """(stride, join) per block of :func:`conv_blocks`, for networks of basic residual blocks (``native_blocks()``
    entries of six: ResNet-18, ResNet-20..56): ``stride[bi]`` = 1 | 2 of the block's 3x3 convolution; ``join[bi]`` =
    None, or (k, sc_conv, sc_bn) for the last block of a branch, whose BatchNorm apply is relu(a*y + b + s) with s
    the output of block k (sc_conv None: identity shortcut), sc_bn(sc_conv(that output)) (1x1 / stride 2
    projection) or, for (k, PAD, None), that output subsampled by 2 and zero-padded by a quarter of the channels on
    each side (option A).  All 1 and None for every other network."""
    nb = model.native_blocks() if hasattr(model, "native_blocks") else ()
    if not nb or len(nb[0]) < 6:
        n = len(conv_blocks(model)[0])
        return [1] * n, [None] * n
    return [b[4] for b in nb], [b[5] for b in nb]


def conv_adds(model):
    """``add[bi]`` per block of :func:`conv_blocks`, for pre-activation networks (``native_blocks()`` entries of
    seven): None, or (k, sc_conv) for a convolution whose raw output y becomes z = y + s before the block's
    BatchNorm, s the pre-BatchNorm tensor of block k (sc_conv None: identity shortcut) or sc_conv(output of block k)
    (1x1 / stride-2 projection, no BatchNorm).  All None for every other network."""
    nb = model.native_blocks() if hasattr(model, "native_blocks") else ()
    if not nb or len(nb[0]) < 7:
        return [None] * len(conv_blocks(model)[0])
    return [b[6] for b in nb]


def deepnn_blocks(model):
    """(blocks, lin0, drop, lin1) of DeepNN: ``blocks[bi] = (conv, pool)`` of its conv + bias -> ReLU [-> pool]
    features, and the classifier's Linear -> ReLU -> Dropout -> Linear modules."""
    mods = list(model.features.children())
    blocks, i = [], 0
    while i < len(mods):
        conv = mods[i]
        assert isinstance(conv, nn.Conv2d) and conv.bias is not None and isinstance(mods[i + 1], nn.ReLU)
        i += 2  # conv, relu
        pool = i < len(mods) and isinstance(mods[i], nn.MaxPool2d)
        if pool:
            i += 1
        blocks.append((conv, pool))
    cls = list(model.classifier.children())
    lin0, drop, lin1 = cls[0], cls[2], cls[3]
    assert isinstance(lin0, nn.Linear) and isinstance(drop, nn.Dropout) and isinstance(lin1, nn.Linear)
    return blocks, lin0, drop, lin1


class DeepNNPlanBase:
    """The part of DeepNN's plan that both precisions share: the walk, the identity affine (a = 1, b = 0) that runs
    the pool and its backward through the BatchNorm kernels, and the dropout generator state."""

    def __init__(self, model):
        self.blocks, self.lin0, self.drop, self.lin1 = deepnn_blocks(model)
        dev = self.lin0.weight.device
        cmax = max(c.weight.shape[0] for c, _ in self.blocks)
        self.ones = torch.ones(cmax, dtype=torch.float32, device=dev)
        self.zeros = torch.zeros(cmax, dtype=torch.float32, device=dev)
        # dropout generator state on the device: [seed, offset] (+ workgroup completion counter)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
        self.rng_done = torch.zeros(1, dtype=torch.int32, device=dev)


def plan_of(model, attr, make):
    """The model's plan stored under ``attr``, made by ``make(model)`` at first use."""
    p = getattr(model, attr, None)
    if p is None:
        p = make(model)
        setattr(model, attr, p)
    return p


def _sync_comm(model, training):
    """The communicator of native SyncBatchNorm (``--sync_bn`` under DDP at world size > 1), or None: batch
    statistics are then merged across ranks inside the forward and the backward (``ops/conv.py`` bn_*_sync,
    ``ops/f32.py`` bn_forward / bn_backward with ``comm``)."""
    comm = getattr(model, "sync_bn_comm", None)
    if training and comm is not None and comm.world_size > 1:
        return comm
    return None
