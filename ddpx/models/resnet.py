"""The model zoo's residual networks: ResNet-9 for CIFAR (the DAWNBench / Myrtle network), described here, the
CIFAR ResNet-18 of basic blocks (:class:`ResNet18`), the CIFAR ResNet-20/32/44/56 with parameter-free option-A
shortcuts (:class:`ResNetCifar`) and the pre-activation ResNet-18/34 (:class:`PreActResNet`, at the end of the file).

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
kernels (VGG's graphs, which follow the skip connections of ``native_blocks()``: ``ddpx.ops.vgg_native`` in bf16,
``ddpx.ops.f32_native`` in fp32) with the skip connection inside the
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
        self.native_dtype = "bf16"  # "bf16" (NHWC bf16 MFMA kernels, fp32 masters) or "fp32" (ddpx.ops.f32_native)

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
                from ..ops import f32_native
                return f32_native.resnet_loss(self, x, targets, soft), None
            from ..ops import vgg_native
            return vgg_native.vgg_loss(self, x, targets, soft), None
        logits = self.forward(x)
        from ..ops.loss import soft_cross_entropy
        return soft_cross_entropy(logits, targets, soft), logits

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._native_ok(x):
            if self.native_dtype == "fp32":
                from ..ops import f32_native
                return f32_native.resnet_forward(self, x)
            from ..ops import vgg_native
            return vgg_native.vgg_forward(self, x)
        x = self.layer1(self.prep(x))
        x = x + self.res1(x)
        x = self.layer3(self.layer2(x))
        x = x + self.res3(x)
        # [N, 512, 4, 4] => [N, 512] => [N, num_classes]
        if self.tail == "max":
            return self.classifier(F.max_pool2d(x, x.shape[-2:]).flatten(1) * self.tail_scale)
        return self.classifier(x.mean([2, 3]))


# ---------------------------------------------------------------------------------------------- ResNet-18
class BasicBlock(nn.Module):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + s), s = x, or sc_bn(sc_conv(x)) when the block downsamples (conv1 and
    the 1x1 sc_conv at stride 2).  Registration order: conv1, bn1, conv2, [sc_conv,] bn2 [, sc_bn] — see
    :class:`ResNet18`."""

    def __init__(self, ci: int, co: int, stride: int = 1) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(co)
        self.conv2 = nn.Conv2d(co, co, 3, padding=1, bias=False)
        self.project = stride != 1 or ci != co
        if self.project:
            self.sc_conv = nn.Conv2d(ci, co, 1, stride=stride, bias=False)
        self.bn2 = nn.BatchNorm2d(co)
        if self.project:
            self.sc_bn = nn.BatchNorm2d(co)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu(out + (self.sc_bn(self.sc_conv(x)) if self.project else x))


_BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _state_keys18():
    keys = ["stem.conv.weight"] + [f"stem.bn.{k}" for k in _BN_KEYS]
    for stage in (1, 2, 3, 4):
        for i in (0, 1):
            b = f"layer{stage}.{i}"
            proj = stage > 1 and i == 0
            keys.append(f"{b}.conv1.weight")
            keys += [f"{b}.bn1.{k}" for k in _BN_KEYS]
            keys.append(f"{b}.conv2.weight")
            if proj:
                keys.append(f"{b}.sc_conv.weight")
            keys += [f"{b}.bn2.{k}" for k in _BN_KEYS]
            if proj:
                keys += [f"{b}.sc_bn.{k}" for k in _BN_KEYS]
    return tuple(keys + ["classifier.weight", "classifier.bias"])


class ResNet18(nn.Module):
    """The CIFAR ResNet-18 (He et al. 2016, the 3x3 stem without max-pool that CIFAR implementations use):

        stem   : conv3x3 3->64, bn, relu                                   32x32
        layer1 : 2 basic blocks, 64 channels, identity shortcuts           32x32
        layer2 : 2 basic blocks, 128; the first: 3x3 / s2, shortcut 1x1 / s2 + bn   16x16
        layer3 : the same at 256                                           8x8
        layer4 : the same at 512                                           4x4
        tail   : x.mean([2, 3]) -> Linear(512, num_classes)

    Every convolution is bias-free.  11,173,962 parameters at 10 classes (counted on this module).

    Registration order, which is the order of the native forward: stem.conv, stem.bn, then per block conv1, bn1,
    conv2, [sc_conv,] bn2 [, sc_bn], then the classifier.  The native backward finishes a block's gradients in the
    reverse of that: the join's merges give sc_bn, then bn2 (both BatchNorms' sums come out of one pass, the shortcut's
    merge runs first), then the weight gradients of sc_conv and conv2, then bn1, conv1 — so grad-ready order is the
    reverse of registration order, which is what DDP's buckets, ZeRO-1 and the overlapped optimizer assume
    (``ops/vgg_native.py``).  This is why sc_conv is registered before bn2.

    Execution: fp32 torch ops on the CPU, with ``--kernels torch`` and with ``--dtype fp32`` (no fp32 join kernels
    yet); in bf16 on MI355X the network runs on VGG's native graph (``ddpx.ops.vgg_native``): strided 3x3 and 1x1
    convolutions, and every block's add + ReLU (and the shortcut's BatchNorm) inside the join kernels
    (``csrc/kernels/bn_join.hip``).  Native SyncBatchNorm is refused: the join's sums would need an all-reduce
    between its passes.
    """
    STATE_KEYS = _state_keys18()

    def __init__(self, num_classes: int = 10) -> None:
        super().__init__()
        self.stem = _block(3, 64)
        ci = 64
        for stage, co in enumerate((64, 128, 256, 512), 1):
            setattr(self, f"layer{stage}", nn.Sequential(BasicBlock(ci, co, 1 if stage == 1 else 2),
                                                         BasicBlock(co, co)))
            ci = co
        self.classifier = nn.Linear(512, num_classes)
        self.use_native = False
        self.native_dtype = "bf16"  # the only native precision
        self._sync_bn_comm = None

    @property
    def sync_bn_comm(self):
        return self._sync_bn_comm

    @sync_bn_comm.setter
    def sync_bn_comm(self, comm):
        if comm is not None and self.use_native:
            raise ValueError("SyncBatchNorm (--sync_bn) is not available for resnet18 on the native kernels: the "
                             "sums of the join kernels would need an all-reduce between their passes; use "
                             "--kernels torch")
        self._sync_bn_comm = comm

    def basic_blocks(self):
        return [b for stage in (1, 2, 3, 4) for b in getattr(self, f"layer{stage}")]

    def native_blocks(self):
        """[(conv, bn, pool, skip, stride, join)] in forward order for the native graph: the stem, then two entries
        per basic block, (conv1, bn1) at the block's stride and (conv2, bn2) whose BatchNorm apply is the join:
        ``join`` = (k, sc_conv, sc_bn) with k the index of the entry whose output is the block's input and
        sc_conv / sc_bn None for an identity shortcut.  ``pool`` is False and ``skip`` None throughout (ResNet-9's
        add-after-ReLU form)."""
        out = [(self.stem.conv, self.stem.bn, False, None, 1, None)]
        for b in self.basic_blocks():
            k = len(out) - 1
            out.append((b.conv1, b.bn1, False, None, b.conv1.stride[0], None))
            out.append((b.conv2, b.bn2, False, None, 1,
                        (k, b.sc_conv, b.sc_bn) if b.project else (k, None, None)))
        return out

    # ---- ddpx engine protocol (as VGG) ------------------------------------------
    def native_active(self, device) -> bool:
        return torch.device(device).type == "cuda" and self.use_native

    def ddpx_spec(self, device):
        if self.native_active(device):
            from ..runtime import native
            native.kernels()  # fail loudly if the extension is missing on a GPU
            return {"shadow_dtype": torch.bfloat16, "native_params": list(self.parameters())}
        return {}

    def input_layout(self, device) -> str:
        return "nhwc8_bf16" if self.native_active(device) else "nchw_f32"

    def _native_ok(self, x):
        return (self.use_native and x.is_cuda and not x.requires_grad
                and getattr(self.classifier.weight, "_ddpx_shadow", None) is not None)

    def forward_loss(self, x: torch.Tensor, targets: torch.Tensor, soft=None):
        """Fused forward + mean cross-entropy on the native path (torch ops otherwise), as :class:`ResNet9`."""
        if self._native_ok(x):
            from ..ops import vgg_native
            return vgg_native.vgg_loss(self, x, targets, soft), None
        logits = self.forward(x)
        from ..ops.loss import soft_cross_entropy
        return soft_cross_entropy(logits, targets, soft), logits

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._native_ok(x):
            from ..ops import vgg_native
            return vgg_native.vgg_forward(self, x)
        x = self.stem(x)
        for stage in (1, 2, 3, 4):
            x = getattr(self, f"layer{stage}")(x)
        return self.classifier(x.mean([2, 3]))


# ---------------------------------------------------------------------------------------------- ResNet-20/32/44/56
class PadBlock(nn.Module):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + s) with the parameter-free shortcut of He et al.'s CIFAR networks
    (option A): s = x, or, when the block downsamples (conv1 at stride 2, co = 2 ci), x subsampled by 2 and
    zero-padded by co/4 channels on each side.  Registration order: conv1, bn1, conv2, bn2."""

    def __init__(self, ci: int, co: int, stride: int = 1) -> None:
        super().__init__()
        if (stride, co) not in ((1, ci), (2, 2 * ci)):
            raise ValueError(f"option-A block: {ci}->{co} at stride {stride} (same width, or doubled at stride 2)")
        self.conv1 = nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(co)
        self.conv2 = nn.Conv2d(co, co, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(co)
        self.pad = 0 if stride == 1 else co // 4

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        s = F.pad(x[:, :, ::2, ::2], (0, 0, 0, 0, self.pad, self.pad)) if self.pad else x
        return F.relu(out + s)


CIFAR_DEPTHS = (20, 32, 44, 56)


def _state_keys_cifar(n: int):
    keys = ["stem.conv.weight"] + [f"stem.bn.{k}" for k in _BN_KEYS]
    for stage in (1, 2, 3):
        for i in range(n):
            for c in (1, 2):
                keys.append(f"layer{stage}.{i}.conv{c}.weight")
                keys += [f"layer{stage}.{i}.bn{c}.{k}" for k in _BN_KEYS]
    return tuple(keys + ["classifier.weight", "classifier.bias"])


class ResNetCifar(ResNet18):
    """The CIFAR residual networks of He et al. 2016, depth 6n+2 (ResNet-20/32/44/56: n = 3/5/7/9):

        stem   : conv3x3 3->16, bn, relu                                   32x32
        layer1 : n basic blocks, 16 channels, identity shortcuts           32x32
        layer2 : n basic blocks, 32; the first: 3x3 / s2 and the option-A shortcut   16x16
        layer3 : the same at 64                                            8x8
        tail   : x.mean([2, 3]) -> Linear(64, num_classes)

    Every convolution is bias-free and the shortcuts have no parameters.  ResNet-20 has 269,722 parameters at 10
    classes (convolutions 267,696, 19 BatchNorms 1,376, head 650).

    Registration order, engine protocol, the fp32 / SyncBatchNorm behaviour and ``native_blocks()`` are ResNet-18's
    (conv1, bn1, conv2, bn2 per block: grad-ready order is the reverse registration order).  On the native bf16
    graph the join of a downsampling block reads the block's input and gathers the shortcut inside the kernel
    (``bn_join(pad=)``); its backward returns the skip gradient compact, and the join below takes it as
    ``gout2_sub`` (``csrc/kernels/bn_join.hip``, ``ops/vgg_native.py``)."""
    STATE_KEYS = _state_keys_cifar(3)  # ResNet-20's; an instance of another depth carries its own

    def __init__(self, depth: int = 20, num_classes: int = 10) -> None:
        if depth < 8 or (depth - 2) % 6:
            raise ValueError(f"ResNetCifar depth must be 6n+2 with n >= 1, got {depth}")
        nn.Module.__init__(self)
        self.depth, self.n = depth, (depth - 2) // 6
        self.STATE_KEYS = _state_keys_cifar(self.n)
        self.stem = _block(3, 16)
        ci = 16
        for stage, co in enumerate((16, 32, 64), 1):
            setattr(self, f"layer{stage}", nn.Sequential(
                *[PadBlock(ci if i == 0 else co, co, 2 if (i == 0 and stage > 1) else 1) for i in range(self.n)]))
            ci = co
        self.classifier = nn.Linear(64, num_classes)
        self.use_native = False
        self.native_dtype = "bf16"  # the only native precision
        self._sync_bn_comm = None

    @property
    def sync_bn_comm(self):
        return self._sync_bn_comm

    @sync_bn_comm.setter
    def sync_bn_comm(self, comm):
        if comm is not None and self.use_native:
            raise ValueError(f"SyncBatchNorm (--sync_bn) is not available for resnet{self.depth} on the native "
                             "kernels: the sums of the join kernels would need an all-reduce between their passes; "
                             "use --kernels torch")
        self._sync_bn_comm = comm

    def basic_blocks(self):
        return [b for stage in (1, 2, 3) for b in getattr(self, f"layer{stage}")]

    def native_blocks(self):
        """As :meth:`ResNet18.native_blocks`; the join of a downsampling block is (k, plan.PAD, None)."""
        from ..ops.plan import PAD
        out = [(self.stem.conv, self.stem.bn, False, None, 1, None)]
        for b in self.basic_blocks():
            k = len(out) - 1
            out.append((b.conv1, b.bn1, False, None, b.conv1.stride[0], None))
            out.append((b.conv2, b.bn2, False, None, 1, (k, PAD if b.pad else None, None)))
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._native_ok(x):
            from ..ops import vgg_native
            return vgg_native.vgg_forward(self, x)
        x = self.stem(x)
        for stage in (1, 2, 3):
            x = getattr(self, f"layer{stage}")(x)
        return self.classifier(x.mean([2, 3]))


# ---------------------------------------------------------------------------------------------- pre-activation
class PreActBlock(nn.Module):
    """z = conv2(relu(bn2(conv1(act)))) + s with act = relu(bn1(x)); s = x, or sc_conv(act) when the block downsamples
    (conv1 and the 1x1 sc_conv at stride 2; the shortcut has no BatchNorm and reads the pre-activated tensor).
    Registration order: bn1, conv1, bn2, conv2 [, sc_conv] — see :class:`PreActResNet`."""

    def __init__(self, ci: int, co: int, stride: int = 1) -> None:
        super().__init__()
        self.bn1 = nn.BatchNorm2d(ci)
        self.conv1 = nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(co)
        self.conv2 = nn.Conv2d(co, co, 3, padding=1, bias=False)
        self.project = stride != 1 or ci != co
        if self.project:
            self.sc_conv = nn.Conv2d(ci, co, 1, stride=stride, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        act = F.relu(self.bn1(x))
        out = self.conv2(F.relu(self.bn2(self.conv1(act))))
        return out + (self.sc_conv(act) if self.project else x)


PREACT_DEPTHS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def _state_keys_preact(counts):
    keys = ["stem.conv.weight"]
    for stage, n in enumerate(counts, 1):
        for i in range(n):
            b = f"layer{stage}.{i}"
            keys += [f"{b}.bn1.{k}" for k in _BN_KEYS]
            keys.append(f"{b}.conv1.weight")
            keys += [f"{b}.bn2.{k}" for k in _BN_KEYS]
            keys.append(f"{b}.conv2.weight")
            if stage > 1 and i == 0:
                keys.append(f"{b}.sc_conv.weight")
    return tuple(keys + [f"bn.{k}" for k in _BN_KEYS] + ["classifier.weight", "classifier.bias"])


class PreActResNet(ResNet18):
    """The pre-activation ResNet-18 / ResNet-34 for CIFAR (He et al. 2016, "Identity Mappings in Deep Residual
    Networks"; blocks 2,2,2,2 / 3,4,6,3):

        stem   : conv3x3 3->64 (no BatchNorm of its own)                   32x32
        layer1 : pre-activation blocks, 64 channels, identity shortcuts    32x32
        layer2 : 128; the first block: 3x3 / s2, shortcut 1x1 / s2 of the pre-activated input   16x16
        layer3 : the same at 256                                           8x8
        layer4 : the same at 512                                           4x4
        tail   : relu(bn(z)).mean([2, 3]) -> Linear(512, num_classes)

    Every convolution is bias-free.  Depth 18 has 11,172,170 parameters at 10 classes (ResNet-18's convolutions and
    head with 7,808 BatchNorm parameters instead of 9,600).

    Registration order: stem.conv, then per block bn1, conv1, bn2, conv2 [, sc_conv], then bn and the classifier.
    Read as dataflow the network is still a chain of conv -> BatchNorm -> ReLU units — (stem, block 1's bn1), (conv1,
    bn2), (conv2, the next block's bn1), ..., (the last conv2, bn) — with an add between a conv2 and the BatchNorm
    after it, which is how ``native_blocks()`` describes it.  The native backward of the unit (conv2, next bn1)
    finishes that BatchNorm, then sc_conv, then conv2; then bn2, conv1; then bn1: the reverse of the registration
    order, as DDP's buckets, ZeRO-1 and the overlapped optimizer assume.  This is why sc_conv is registered last.

    Engine protocol, fp32 and SyncBatchNorm behaviour are ResNet-18's (fp32 runs the torch ops; native SyncBatchNorm is
    refused).  On the native bf16 graph a unit with an add runs ``conv_fwd(stats=False)`` -> ``preact_add`` (the add
    and the statistics of the sum, ``csrc/kernels/bn_preact.hip``) -> ``bn_finalize`` -> ``bn_apply``, and its
    BatchNorm backward adds the gradient that the identity shortcut carries on its output side
    (``bn_backward(gadd=)``) or, below a projection, takes the 1x1 data gradient as ``gout2``."""
    STATE_KEYS = _state_keys_preact(PREACT_DEPTHS[18])  # depth 18's; an instance of another depth carries its own

    def __init__(self, depth: int = 18, num_classes: int = 10) -> None:
        if depth not in PREACT_DEPTHS:
            raise ValueError(f"PreActResNet depth must be one of {sorted(PREACT_DEPTHS)}, got {depth}")
        nn.Module.__init__(self)
        self.depth, self.counts = depth, PREACT_DEPTHS[depth]
        self.STATE_KEYS = _state_keys_preact(self.counts)
        self.stem = nn.Sequential(OrderedDict([("conv", nn.Conv2d(3, 64, 3, padding=1, bias=False))]))
        ci = 64
        for stage, (co, n) in enumerate(zip((64, 128, 256, 512), self.counts), 1):
            setattr(self, f"layer{stage}", nn.Sequential(
                *[PreActBlock(ci if i == 0 else co, co, 2 if (i == 0 and stage > 1) else 1) for i in range(n)]))
            ci = co
        self.bn = nn.BatchNorm2d(512)
        self.classifier = nn.Linear(512, num_classes)
        self.use_native = False
        self.native_dtype = "bf16"  # the only native precision
        self._sync_bn_comm = None

    @property
    def sync_bn_comm(self):
        return self._sync_bn_comm

    @sync_bn_comm.setter
    def sync_bn_comm(self, comm):
        if comm is not None and self.use_native:
            raise ValueError(f"SyncBatchNorm (--sync_bn) is not available for preact_resnet{self.depth} on the native "
                             "kernels: the statistics of the shortcut add have no cross-rank merge in the graph yet; "
                             "use --kernels torch")
        self._sync_bn_comm = comm

    def native_blocks(self):
        """[(conv, bn, pool, skip, stride, join, add)] in forward order for the native graph: unit (conv, the
        BatchNorm that reads its output).  ``add`` = None, or (k, sc_conv) for a block's conv2: its raw output y
        becomes z = y + s before the BatchNorm, s the pre-BatchNorm tensor of unit k (sc_conv None: the identity
        shortcut, the previous block's z) or sc_conv(output of unit k) (the 1x1 / stride-2 projection of the
        pre-activated input).  ``pool`` False, ``skip`` and ``join`` None throughout."""
        blocks = self.basic_blocks()
        bns = [b.bn1 for b in blocks[1:]] + [self.bn]
        out = [(self.stem.conv, blocks[0].bn1, False, None, 1, None, None)]
        for b, bn_next in zip(blocks, bns):
            k = len(out) - 1
            out.append((b.conv1, b.bn2, False, None, b.conv1.stride[0], None, None))
            out.append((b.conv2, bn_next, False, None, 1, None, (k, b.sc_conv if b.project else None)))
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._native_ok(x):
            from ..ops import vgg_native
            return vgg_native.vgg_forward(self, x)
        x = self.stem(x)
        for stage in (1, 2, 3, 4):
            x = getattr(self, f"layer{stage}")(x)
        return self.classifier(F.relu(self.bn(x)).mean([2, 3]))
