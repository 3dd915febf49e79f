"""ResNet-9 for CIFAR (the DAWNBench / Myrtle network): the model zoo's residual network.

Forward order, which is also the module registration order (conv -> bn -> relu [-> pool], as VGG's ``add()``):

    prep   : conv 3->64      bn relu                  32x32
    layer1 : conv 64->128    bn relu pool2            32x32 -> 16x16
    res1   : x + [conv 128->128 bn relu, conv 128->128 bn relu](x)
    layer2 : conv 128->256   bn relu pool2            16x16 -> 8x8
    layer3 : conv 256->512   bn relu pool2            8x8  -> 4x4
    res3   : x + [conv 512->512 bn relu, conv 512->512 bn relu](x)
    tail   : x.mean([2, 3]) -> Linear(512, num_classes)                       tail="avg" (the default)
             tail_scale * max_pool2d(x, 4).flatten(1) -> Linear(512, ...)    tail="max"

Every convolution is ``nn.Conv2d(ci, co, 3, padding=1, bias=False)``; the add comes after the branch's last ReLU
and no activation follows it.  6,573,130 parameters at 10 classes.

The tail.  The default, ``tail="avg"``, is VGG's (the global-average-pool kernels and the fused classifier head).
The network as published ends in a 4x4 max-pool and scales its logits by 0.125: that is
``ResNet9(tail="max", tail_scale=0.125)`` (``--resnet_tail max --tail_scale 0.125``).  The scale is applied to the
pooled *features*, inside the global max-pool kernels (``ddpx_gmaxpool`` / ``ddpx_f32_gmaxpool``), so the fused head
kernels stay as they are.  For the published bias-free classifier that is the same network exactly,
``0.125 * (W f) = W (0.125 f)`` with a power-of-two scale; this project's classifier keeps its bias, so here the
logits are ``W (s f) + b``: the bias is not scaled.  ``tail_scale != 1`` with ``tail="avg"`` is a ``ValueError``.
The tail has no parameters, so ``STATE_KEYS`` and every checkpoint format are the same for both tails; the full
checkpoint records ``{"tail", "tail_scale"}`` when they are not the defaults (a default run's file is what it
always was; a missing record reads as the default) and ``--resume`` refuses other values.  Still missing against the
published recipe: CELU, ghost BatchNorm, input whitening and the bias-free classifier.

``state_dict`` keys (this project's own checkpoint format): ``{prep,layer1,layer2,layer3}.{conv,bn}.*``,
``{res1,res3}.{0,1}.{conv,bn}.*`` and ``classifier.{weight,bias}`` — see :data:`ResNet9.STATE_KEYS`.

Execution: fp32 torch ops on the CPU (or with ``--kernels torch``); on MI355X the whole network runs on the native
kernels (``ddpx.ops.resnet_native`` in bf16, ``ddpx.ops.f32`` in fp32) with the skip connection inside the
BatchNorm kernels: the add in the apply pass of the branch's last block, the sum of the two gradients that meet
below a residual block inside the BatchNorm backward of that block.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn


def _block(ci: int, co: int, pool: bool = False) -> nn.Sequential:
    layers = [("conv", nn.Conv2d(ci, co, 3, padding=1, bias=False)), ("bn", nn.BatchNorm2d(co)),
              ("relu", nn.ReLU(True))]
    if pool:
        layers.append(("pool", nn.MaxPool2d(2)))
    return nn.Sequential(OrderedDict(layers))


def tail_of(model):
    """(tail, tail_scale) of a model's pooling tail: ("avg", 1.0) for every model that names none.  The one lookup
    the native graphs and the checkpoint share."""
    return str(getattr(model, "tail", "avg")), float(getattr(model, "tail_scale", 1.0))


def _state_keys():
    keys = []
    for blk in ("prep", "layer1", "res1.0", "res1.1", "layer2", "layer3", "res3.0", "res3.1"):
        keys.append(f"{blk}.conv.weight")
        keys += [f"{blk}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return tuple(keys + ["classifier.weight", "classifier.bias"])


class ResNet9(nn.Module):
    STATE_KEYS = _state_keys()

    def __init__(self, num_classes: int = 10, tail: str = "avg", tail_scale: float = 1.0) -> None:
        super().__init__()
        if tail not in ("avg", "max"):
            raise ValueError(f"tail must be 'avg' or 'max', got {tail!r}")
        tail_scale = float(tail_scale)
        if not math.isfinite(tail_scale):
            raise ValueError(f"tail_scale must be finite, got {tail_scale}")
        if tail == "avg" and tail_scale != 1.0:
            raise ValueError("tail_scale applies to tail='max' only (the average tail has no feature scale)")
        # the tail has no parameters: plain attributes, not in the state_dict (the full checkpoint records them)
        self.tail, self.tail_scale = tail, tail_scale
        self.prep = _block(3, 64)
        self.layer1 = _block(64, 128, pool=True)
        self.res1 = nn.Sequential(_block(128, 128), _block(128, 128))
        self.layer2 = _block(128, 256, pool=True)
        self.layer3 = _block(256, 512, pool=True)
        self.res3 = nn.Sequential(_block(512, 512), _block(512, 512))
        self.classifier = nn.Linear(512, num_classes)
        self.use_native = False
        self.native_dtype = "bf16"  # "bf16" (NHWC bf16 MFMA kernels, fp32 masters) or "fp32" (ddpx.ops.f32)

    def native_blocks(self):
        """[(conv, bn, pool, skip)] in forward order for the native graphs; ``skip`` = index of the block whose
        output is added to this block's output (the last block of a residual branch), else None."""
        seq = [self.prep, self.layer1, self.res1[0], self.res1[1], self.layer2, self.layer3, self.res3[0],
               self.res3[1]]
        skip = {3: 1, 7: 5}
        return [(b.conv, b.bn, hasattr(b, "pool"), skip.get(i)) for i, b in enumerate(seq)]

    # ---- ddpx engine protocol (as VGG) ------------------------------------------
    def native_active(self, device) -> bool:
        return torch.device(device).type == "cuda" and self.use_native

    def ddpx_spec(self, device):
        if self.native_active(device):
            from ..runtime import native
            native.kernels()  # fail loudly if the extension is missing on a GPU
            if self.native_dtype == "fp32":
                return {"native_params": list(self.parameters())}
            return {"shadow_dtype": torch.bfloat16, "native_params": list(self.parameters())}
        return {}

    def input_layout(self, device) -> str:
        if not self.native_active(device):
            return "nchw_f32"
        return "nhwc4_f32" if self.native_dtype == "fp32" else "nhwc8_bf16"

    def _native_ok(self, x):
        if not (self.use_native and x.is_cuda and not x.requires_grad):
            return False
        if self.native_dtype == "fp32":
            return getattr(self.classifier.weight, "_ddpx_flat", None) is not None
        return getattr(self.classifier.weight, "_ddpx_shadow", None) is not None

    def forward_loss(self, x: torch.Tensor, targets: torch.Tensor, soft=None):
        """Fused forward + mean cross-entropy on the native path (torch ops otherwise).  ``soft``
        (:class:`ddpx.ops.loss.SoftTargets`): label smoothing / Mixup-CutMix second labels."""
        if self._native_ok(x):
            if self.native_dtype == "fp32":
                from ..ops import f32
                return f32.resnet_loss(self, x, targets, soft), None
            from ..ops import resnet_native
            return resnet_native.resnet_loss(self, x, targets, soft), None
        logits = self.forward(x)
        from ..ops.loss import soft_cross_entropy
        return soft_cross_entropy(logits, targets, soft), logits

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._native_ok(x):
            if self.native_dtype == "fp32":
                from ..ops import f32
                return f32.resnet_forward(self, x)
            from ..ops import resnet_native
            return resnet_native.resnet_forward(self, x)
        x = self.layer1(self.prep(x))
        x = x + self.res1(x)
        x = self.layer3(self.layer2(x))
        x = x + self.res3(x)
        # [N, 512, 4, 4] => [N, 512] => [N, num_classes]
        if self.tail == "max":
            return self.classifier(F.max_pool2d(x, x.shape[-2:]).flatten(1) * self.tail_scale)
        return self.classifier(x.mean([2, 3]))
