"""Host wrappers of the weight-EMA kernels (``csrc/kernels/ema.hip``) and the host twin of the advance kernel."""
from __future__ import annotations

import torch

from ..runtime import native


def _f32(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


def ema_weight(step: int, updates: int, decay: float, warmup: bool, every: int):
    """The host twin of ``ema_advance_kernel``: ``step`` is the 1-based number of the optimizer step being taken,
    ``updates`` the number of EMA updates before it.  Returns ``(updates after it, w)`` with ``w`` rounded once to
    fp32: 0 on a step that is no multiple of ``every``, else ``1 - d^every`` with
    ``d = min(decay, (1 + u) / (10 + u))`` under warm-up (``u``: the new update count) and ``d = decay`` without."""
    if not 0.0 <= float(decay) < 1.0 or int(every) < 1:
        raise ValueError("ema_weight: decay in [0, 1) and every >= 1")
    if int(step) % int(every) != 0:
        return int(updates), 0.0
    u = int(updates) + 1
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + u) / (10.0 + u))
    if every > 1:
        d = d ** float(every)
    return u, _f32(1.0 - d)


def ema_advance_(counters: torch.Tensor, decay: float, warmup: bool, every: int, w_out: torch.Tensor):
    """GPU: ``counters`` (int32 [2]: steps, updates) and ``w_out`` (fp32 scalar) advance by one optimizer step in one
    1-thread launch on the current stream (capturable: no host value involved); see :func:`ema_weight`."""
    if not (counters.is_cuda and w_out.is_cuda and counters.dtype == torch.int32 and counters.numel() == 2
            and w_out.dtype == torch.float32 and w_out.numel() == 1):
        raise ValueError("ema_advance: int32 [2] counters and an fp32 scalar weight on the GPU")
    rc = native.kernels().ddpx_ema_advance(counters.data_ptr(), float(decay), int(bool(warmup)), int(every),
                                           w_out.data_ptr(), native.stream_handle())
    native.check(rc, "ddpx_ema_advance")


def ema_flat_(ema: torch.Tensor, p: torch.Tensor, w: float | torch.Tensor):
    """``ema += (p - ema) * w`` over flat contiguous fp32 buffers.

    GPU: ``ddpx_ema_flat``, two roundings per element; ``w`` is a Python float or a 0-d / 1-element fp32 device
    tensor, and a weight of 0 touches nothing (``ema`` stays bit-exact whatever ``p`` holds).  CPU: ``ema.lerp_(p, w)``
    (the same bits as the fma form while ``w < 0.5``; torch switches to ``p - (p - ema) * (1 - w)`` from 0.5 on),
    skipped for ``w == 0``."""
    n = ema.numel()
    if p.numel() != n or ema.dtype != torch.float32 or p.dtype != torch.float32:
        raise ValueError("ema_flat: two fp32 buffers of equal numel")
    if not ema.is_cuda:
        w = float(w.item()) if torch.is_tensor(w) else float(w)
        if w != 0.0:
            ema.lerp_(p, w)
        return ema
    if torch.is_tensor(w) and (w.dtype != torch.float32 or w.device != ema.device or w.numel() != 1):
        raise ValueError("ema_flat: w must be an fp32 scalar on the buffers' device")
    w_dev = w.data_ptr() if torch.is_tensor(w) else None
    w_host = 0.0 if torch.is_tensor(w) else float(w)
    rc = native.kernels().ddpx_ema_flat(ema.data_ptr(), p.data_ptr(), n, w_dev, w_host, native.stream_handle())
    native.check(rc, "ddpx_ema_flat")
    return ema
