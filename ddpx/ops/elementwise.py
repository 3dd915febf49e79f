"""Host wrappers for the memory-bound native kernels (casts, column sums, SGD).

CPU tensors take an equivalent torch path (the CPU is a supported device for
the reference-shaped workloads, BASELINE config 1); GPU tensors always take the
native HIP path.
"""
from __future__ import annotations

import math

import torch

from ..runtime import native


def cast_bf16_(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst (bf16) <- src (fp32), both contiguous with equal numel."""
    if src.numel() != dst.numel():
        raise ValueError("cast: numel mismatch")
    if not src.is_cuda:
        dst.copy_(src.to(torch.bfloat16))
        return dst
    if src.dtype != torch.float32 or dst.dtype != torch.bfloat16:
        raise ValueError("cast: expected fp32 -> bf16")
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("cast: tensors must be contiguous")
    lib = native.kernels()
    native.check(lib.ddpx_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), native.stream_handle()),
                 "ddpx_cast_f32_bf16")
    return dst


def colsum_bf16(x: torch.Tensor, out: torch.Tensor, scale: float = 1.0, accumulate: bool = False):
    """out[n] (=|+=) scale * sum_m x[m, n]   (bias gradient of a Linear)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("colsum: x must be a row-contiguous 2-D tensor")
    M, N = x.shape
    if out.numel() != N or out.dtype != torch.float32:
        raise ValueError("colsum: out must be fp32 [N]")
    if not x.is_cuda:
        s = x.float().sum(0) * scale
        if accumulate:
            out.add_(s.view_as(out))
        else:
            out.copy_(s.view_as(out))
        return out
    if x.dtype != torch.bfloat16:
        raise ValueError("colsum: x must be bf16 on GPU")
    lib = native.kernels()
    native.check(lib.ddpx_colsum_bf16(x.data_ptr(), out.data_ptr(), M, N, x.stride(0), float(scale),
                                      int(accumulate), native.stream_handle()), "ddpx_colsum_bf16")
    return out


def sgd_flat_(param: torch.Tensor, momentum_buf: torch.Tensor, grad: torch.Tensor, shadow: torch.Tensor | None,
              lr: float | torch.Tensor, momentum: float, weight_decay: float, grad_scale: float = 1.0,
              nesterov: bool = False, first: bool = False, mx8=None, clip: torch.Tensor | None = None):
    """One fused SGD step over flat contiguous buffers (torch.optim.SGD semantics, dampening=0).

    ``lr`` may be a Python float or a 0-d fp32 device tensor (graph-capturable path).
    ``mx8`` = (codes uint8 [n], E8M0 scales uint8 [n / 32]), n % 32 == 0: also write the updated parameters as
    MX-FP8 e4m3 blocks of 32 consecutive elements (the fp8 forward's weight operand; GPU only).
    ``clip``: a 0-d fp32 tensor on the parameters' device that also scales the gradient (the clip factor of
    ``ddpx.ops.clip.GradNormPlan``, read on the device); a factor of exactly 1.0 changes no bit.
    """
    n = param.numel()
    if momentum_buf.numel() != n or grad.numel() != n or (shadow is not None and shadow.numel() != n):
        raise ValueError("sgd_flat: buffers must have equal numel")
    if not param.is_cuda:
        lr_v = float(lr) if not torch.is_tensor(lr) else float(lr.item())
        if clip is not None:
            grad_scale = grad_scale * float(clip.item())
        # one cache-blocked sweep: each 256K-element block goes through every pass while it is still in
        # L2 (whole-buffer passes with full-size temporaries cost ~3.7x on the 29M-parameter MLP); the
        # per-element arithmetic and its rounding order are torch.optim.SGD's
        blk = 1 << 18
        tmp = torch.empty(min(n, blk), dtype=torch.float32)
        pf, bf, gf = param.view(-1), momentum_buf.view(-1), grad.view(-1)
        sf = shadow.view(-1) if shadow is not None else None
        for s in range(0, n, blk):
            e = min(n, s + blk)
            p, g = pf[s:e], gf[s:e]
            d = tmp[:e - s]
            d.copy_(g)
            if grad_scale != 1.0:
                d.mul_(grad_scale)
            if weight_decay:
                d.add_(p, alpha=weight_decay)
            if momentum:
                b = bf[s:e]
                if first:
                    b.copy_(d)
                else:
                    b.mul_(momentum).add_(d)
                if nesterov:
                    d.add_(b, alpha=momentum)
                else:
                    d = b
            p.add_(d, alpha=-lr_v)
            if sf is not None:
                sf[s:e].copy_(p)
        return param
    lib = native.kernels()
    lr_dev = lr.data_ptr() if torch.is_tensor(lr) else None
    lr_host = 0.0 if torch.is_tensor(lr) else float(lr)
    if clip is not None:
        if clip.dtype != torch.float32 or clip.device != param.device:
            raise ValueError("sgd_flat: clip must be an fp32 scalar on the parameters' device")
        rc = lib.ddpx_sgd_flat_clip(param.data_ptr(), momentum_buf.data_ptr(), grad.data_ptr(),
                                    int(grad.dtype == torch.bfloat16), native.ptr(shadow), n, lr_dev, lr_host,
                                    float(momentum), float(weight_decay), float(grad_scale), clip.data_ptr(),
                                    int(nesterov), int(first), native.ptr(mx8[0] if mx8 else None),
                                    native.ptr(mx8[1] if mx8 else None), native.stream_handle())
        native.check(rc, "ddpx_sgd_flat_clip")
        return param
    rc = lib.ddpx_sgd_flat(param.data_ptr(), momentum_buf.data_ptr(), grad.data_ptr(),
                           int(grad.dtype == torch.bfloat16), native.ptr(shadow), n, lr_dev, lr_host,
                           float(momentum), float(weight_decay), float(grad_scale), int(nesterov), int(first),
                           native.ptr(mx8[0] if mx8 else None), native.ptr(mx8[1] if mx8 else None),
                           native.stream_handle())
    native.check(rc, "ddpx_sgd_flat")
    return param


def adamw_advance_(counter: torch.Tensor, bc: torch.Tensor, beta1: float, beta2: float):
    """GPU: ``counter`` (int32 [1]) += 1 and ``bc`` (fp32 [2]) <- {1 - beta1^t, sqrt(1 - beta2^t)} for the new t,
    in one 1-thread launch on the current stream (capturable: no host value involved)."""
    if not (counter.is_cuda and bc.is_cuda and counter.dtype == torch.int32 and bc.dtype == torch.float32
            and bc.numel() == 2):
        raise ValueError("adamw_advance: int32 [1] counter and fp32 [2] bias corrections on the GPU")
    rc = native.kernels().ddpx_adamw_advance(counter.data_ptr(), float(beta1), float(beta2), bc.data_ptr(),
                                             native.stream_handle())
    native.check(rc, "ddpx_adamw_advance")


def adamw_flat_(param: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, grad: torch.Tensor,
                shadow: torch.Tensor | None, lr: float | torch.Tensor, bc: torch.Tensor | None, step: int | None,
                beta1: float, beta2: float, eps: float, weight_decay: float, grad_scale: float = 1.0,
                clip: torch.Tensor | None = None):
    """One fused AdamW step over flat contiguous buffers (torch.optim.AdamW semantics: decoupled weight decay,
    no amsgrad, no maximize).

    GPU: ``bc`` holds the step's two bias-correction scalars (:func:`adamw_advance_`), ``lr`` is a Python float
    or a 0-d fp32 device tensor, ``step`` is unused.  CPU: ``step`` is the 1-based step number and ``bc`` is
    unused; the sweep is torch's ``_single_tensor_adam`` op by op, so its bits are ``torch.optim.AdamW``'s.
    ``clip``: a 0-d fp32 tensor on the parameters' device that also scales the gradient (the clip factor of
    ``ddpx.ops.clip.GradNormPlan``); a factor of exactly 1.0 changes no bit.
    """
    n = param.numel()
    if (exp_avg.numel() != n or exp_avg_sq.numel() != n or grad.numel() != n
            or (shadow is not None and shadow.numel() != n)):
        raise ValueError("adamw_flat: buffers must have equal numel")
    if not param.is_cuda:
        if step is None or step < 1:
            raise ValueError("adamw_flat: the CPU path needs the 1-based step number")
        lr_v = float(lr) if not torch.is_tensor(lr) else float(lr.item())
        if clip is not None:
            grad_scale = grad_scale * float(clip.item())
        bc1 = 1 - beta1 ** step
        bc2 = 1 - beta2 ** step
        step_size = lr_v / bc1
        bc2s = bc2 ** 0.5
        # one cache-blocked sweep (see sgd_flat_): every 256K-element block goes through all passes while it
        # is in L2; elementwise ops, so blocking changes no bit
        blk = 1 << 18
        scaled = grad_scale != 1.0 or grad.dtype != torch.float32
        gtmp = torch.empty(min(n, blk), dtype=torch.float32) if scaled else None
        denom = torch.empty(min(n, blk), dtype=torch.float32)
        pf, mf, vf, gf = param.view(-1), exp_avg.view(-1), exp_avg_sq.view(-1), grad.view(-1)
        sf = shadow.view(-1) if shadow is not None else None
        for s in range(0, n, blk):
            e = min(n, s + blk)
            p, m, v, g = pf[s:e], mf[s:e], vf[s:e], gf[s:e]
            if scaled:
                g = gtmp[:e - s].copy_(g)
                if grad_scale != 1.0:
                    g.mul_(grad_scale)
            if weight_decay != 0:
                p.mul_(1 - lr_v * weight_decay)
            m.lerp_(g, 1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            d = denom[:e - s]
            torch.sqrt(v, out=d)
            d.div_(bc2s).add_(eps)
            p.addcdiv_(m, d, value=-step_size)
            if sf is not None:
                sf[s:e].copy_(p)
        return param
    if bc is None or not bc.is_cuda or bc.dtype != torch.float32 or bc.numel() != 2:
        raise ValueError("adamw_flat: bc must be the fp32 [2] device tensor of adamw_advance_")
    if clip is not None and (clip.dtype != torch.float32 or clip.device != param.device):
        raise ValueError("adamw_flat: clip must be an fp32 scalar on the parameters' device")
    lr_dev = lr.data_ptr() if torch.is_tensor(lr) else None
    lr_host = 0.0 if torch.is_tensor(lr) else float(lr)
    rc = native.kernels().ddpx_adamw_flat(param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                          grad.data_ptr(), int(grad.dtype == torch.bfloat16), native.ptr(shadow), n,
                                          lr_dev, lr_host, bc.data_ptr(), float(beta1), float(beta2), float(eps),
                                          float(weight_decay), float(grad_scale), native.ptr(clip),
                                          native.stream_handle())
    native.check(rc, "ddpx_adamw_flat")
    return param


_NHWC_LAYOUTS = ("nhwc_bf16", "nhwc_f32", "nhwc8_bf16", "nhwc4_f32")
_HFLIP_LAYOUTS = ("nchw_f32", "nchw_bf16", "flat_f32", "flat_bf16") + _NHWC_LAYOUTS


def hflip(x: torch.Tensor, layout: str, width: int | None = None) -> torch.Tensor:
    """The mirror image (left-right) of a batch in a loader layout (``ddpx.data.loader.LAYOUTS``), as a new tensor:
    ``torch.flip`` along the image's W axis, one ``ddpx_hflip`` launch on the GPU.  ``width``: the image width of a
    flat layout ([N, C*H*W]; default: square 3-channel images)."""
    if layout not in _HFLIP_LAYOUTS:
        raise ValueError(f"hflip: unknown layout {layout!r}")
    want = torch.bfloat16 if "bf16" in layout else torch.float32
    if x.dtype != want or not x.is_contiguous():
        raise ValueError(f"hflip: a contiguous {want} tensor expected for {layout}")
    if layout.startswith("flat"):
        if x.dim() != 2:
            raise ValueError("hflip: a flat batch is [N, C*H*W]")
        W = int(width) if width else math.isqrt(x.shape[1] // 3)
        if not width and 3 * W * W != x.shape[1]:
            raise ValueError(f"hflip: a flat row of {x.shape[1]} elements is no square 3-channel image: pass width")
        if W < 1 or x.shape[1] % W:
            raise ValueError(f"hflip: row length {x.shape[1]} is no multiple of the image width {W}")
        wdim, E = None, x.element_size()
    elif x.dim() != 4:
        raise ValueError(f"hflip: {layout} batches are 4-D")
    elif layout in _NHWC_LAYOUTS:
        wdim, W, E = 2, x.shape[2], x.shape[3] * x.element_size()
    else:
        wdim, W, E = 3, x.shape[3], x.element_size()
    if not x.is_cuda:
        return (x.view(x.shape[0], -1, W).flip(2).reshape(x.shape) if wdim is None else x.flip(wdim)).contiguous()
    out = torch.empty_like(x)
    R = x.numel() * x.element_size() // (W * E)
    native.check(native.kernels().ddpx_hflip(x.data_ptr(), R, W, E, out.data_ptr(), native.stream_handle()),
                 "ddpx_hflip")
    return out


def scale_(x: torch.Tensor, s: float):
    if not x.is_cuda or x.dtype != torch.float32:
        return x.mul_(s)
    lib = native.kernels()
    native.check(lib.ddpx_scale_f32(x.data_ptr(), x.numel(), float(s), native.stream_handle()), "ddpx_scale_f32")
    return x
