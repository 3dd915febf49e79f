"""Model zoo: the reference's VGG and DeepNN, the BASELINE MLPs, and ResNet-9."""
from __future__ import annotations

import torch

from .deepnn import DeepNN
from .mlp import MLP
from .resnet import ResNet9
from .vgg import VGG

__all__ = ["VGG", "DeepNN", "MLP", "ResNet9", "build_model", "native_kernels_for"]


def native_kernels_for(name: str, dtype: str, kernels: str = "auto") -> bool:
    """Whether ``build_model`` puts ``name`` on the hand-written kernels for ``kernels`` = auto|native|torch.

    auto = native everywhere (measured faster than the stock libraries on every model and precision, including the
    reference's fp32 recipe: VGG 18.79 vs MIOpen 19.46 ms, DeepNN 3.83 vs 4.29 ms per step, profiles/r4_f32);
    ``--kernels torch`` runs the torch/MIOpen ops under the ddpx engine (flat store, fused flat SGD, native DDP)."""
    if kernels == "torch":
        return False
    if kernels == "native":
        return True
    # measured (profiles/r4_f32): at fp32 the native kernels beat MIOpen on both CNNs (VGG 18.79 vs 19.46 ms,
    # DeepNN 3.83 vs 4.29 ms per step, same boxes), so auto is native everywhere
    return True


def build_model(name: str, hidden=None, layers: int = 3, dtype: str = "auto", device=None, kernels: str = "auto",
                fp8: bool = False, num_classes: int = 10, tail: str = "avg", tail_scale: float = 1.0):
    """``tail`` / ``tail_scale``: ResNet-9's pooling tail (``models/resnet.py``); any other model takes the defaults
    only."""
    if name != "resnet9" and (tail != "avg" or float(tail_scale) != 1.0):
        raise ValueError(f"tail / tail_scale apply to resnet9 only, not to {name!r}")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dtype == "auto":
        dtype = "bf16" if dev.type == "cuda" else "fp32"
    cdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    native = native_kernels_for(name, dtype, kernels)
    if name == "vgg":
        m = VGG(num_classes)
        # native NHWC kernels on the GPU: bf16 MFMA, or the exact-f32 MFMA path for the reference's fp32
        m.use_native = native and dev.type == "cuda"
        m.native_dtype = "fp32" if dtype == "fp32" else "bf16"
    elif name == "resnet9":
        m = ResNet9(num_classes, tail=tail, tail_scale=tail_scale)
        m.use_native = native and dev.type == "cuda"
        m.native_dtype = "fp32" if dtype == "fp32" else "bf16"
    elif name == "deepnn":
        m = DeepNN(num_classes)
        m.use_native = native and dev.type == "cuda"
        m.native_dtype = "fp32" if dtype == "fp32" else "bf16"
    elif name in ("mlp", "mlp_wide"):
        h = hidden or (16384 if name == "mlp_wide" else 4096)
        m = MLP(hidden=h, layers=layers, num_classes=num_classes, compute_dtype=cdt)
        m.use_native = native
        m.fp8 = bool(fp8)  # MX-FP8 forward / weight-gradient GEMMs on the native path
    else:
        raise ValueError(f"unknown model {name!r}")
    return m
