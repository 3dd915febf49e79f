"""Host wrappers: 3x3 implicit-GEMM convolutions, BatchNorm/ReLU/MaxPool, average pool (NHWC bf16).

Kernels: ``csrc/kernels/conv_igemm.hip``, ``csrc/kernels/conv_igemm_s2.hip`` (stride 2: 3x3 / pad 1 and 1x1 / pad 0)
, ``csrc/kernels/conv1x1_s1.hip`` (1x1 / stride 1), ``csrc/kernels/bn_pool.hip``, ``csrc/kernels/bn_join.hip``
(the join of a basic residual block) and ``csrc/kernels/bn_preact.hip`` (the shortcut add of a pre-activation block).  Every wrapper checks shapes,
dtypes and contiguity on the host before launching.
"""
from __future__ import annotations

import math

import torch

from ..runtime import native


def _req(c, msg):
    if not c:
        raise ValueError(msg)


def _nhwc(x, name, C=None):
    _req(x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous(), f"{name} must be contiguous bf16 on GPU")
    _req(x.data_ptr() % 16 == 0, f"{name} must be 16-B aligned")
    if C is not None:
        _req(x.shape[-1] == C, f"{name}: expected {C} channels, got {tuple(x.shape)}")


def padded_channels(c: int) -> int:
    return max(8, (c + 7) // 8 * 8)


def weight_prep(w: torch.Tensor, wf: torch.Tensor, wd: torch.Tensor):
    """fp32 torch weight [Co,Ci,3,3] -> wf [Co,9,Cp] and wd [9,Co,Cp] (bf16, zero-padded channels)."""
    Co, Ci = w.shape[0], w.shape[1]
    Cp = padded_channels(Ci)
    _req(tuple(w.shape) == (Co, Ci, 3, 3) and w.dtype == torch.float32 and w.is_contiguous(), "bad conv weight")
    _req(wf.numel() == Co * 9 * Cp and wd.numel() == Co * 9 * Cp, "bad prepared-weight buffers")
    native.check(native.kernels().ddpx_conv_weight_prep(w.data_ptr(), Co, Ci, Cp, wf.data_ptr(), wd.data_ptr(),
                                                        native.stream_handle()), "ddpx_conv_weight_prep")


def conv_fwd(x, wf, Co, stats=True, tile=-1):
    """y [N*H*W, Co] bf16 (+ per-tile BN statistics [T,2,Co] fp32 and tile rows)."""
    N, H, W, C = x.shape
    _nhwc(x, "x")
    _req(C % 8 == 0 and wf.numel() == Co * 9 * C, "conv_fwd: weight/input channel mismatch")
    lib = native.kernels()
    P = N * H * W
    y = torch.empty((P, Co), dtype=torch.bfloat16, device=x.device)
    st, T, BM = None, 0, 0
    if stats:
        T = lib.ddpx_conv_fwd_tiles_m(P, C, Co, tile)
        BM = lib.ddpx_conv_fwd_tile_rows(P, C, Co, tile)
        st = torch.empty((T, 2, Co), dtype=torch.float32, device=x.device)
    native.check(lib.ddpx_conv_fwd(x.data_ptr(), wf.data_ptr(), y.data_ptr(), native.ptr(st), N, H, W, C, Co, tile,
                                   native.stream_handle()), "ddpx_conv_fwd")
    return y, st, T, BM


def conv_fwd_act(x, wf, Co, bias, tile=-1):
    """act [N*H*W, Co] bf16 = relu(conv(x) + bias), bias + ReLU in the GEMM epilogue (DeepNN's conv blocks)."""
    N, H, W, C = x.shape
    _nhwc(x, "x")
    _req(C % 8 == 0 and wf.numel() == Co * 9 * C, "conv_fwd_act: weight/input channel mismatch")
    _req(bias.dtype == torch.float32 and bias.numel() == Co and bias.is_contiguous(), "conv_fwd_act: bias fp32 [Co]")
    act = torch.empty((N * H * W, Co), dtype=torch.bfloat16, device=x.device)
    native.check(native.kernels().ddpx_conv_fwd_act(x.data_ptr(), wf.data_ptr(), act.data_ptr(), bias.data_ptr(),
                                                    N, H, W, C, Co, tile, native.stream_handle()), "ddpx_conv_fwd_act")
    return act


def conv_dgrad_act(dy, wd, N, H, W, C, Co, act, tile=-1):
    """(dz [N*H*W, C] bf16, (part [T, C] fp32, T)): the data gradient masked by the ReLU of the block below
    (``act`` = its relu(conv + bias) output, [N*H*W, C]) in the GEMM epilogue, with per-row-tile column sums of
    dz (that block's bias gradient, finished by :func:`colsum_finish`)."""
    _nhwc(dy, "dy", Co)
    _nhwc(act, "act", C)
    _req(act.numel() == N * H * W * C, "conv_dgrad_act: act must be [N*H*W, C]")
    _req(wd.numel() == 9 * Co * C, "conv_dgrad_act: bad weight buffer")
    lib = native.kernels()
    T = lib.ddpx_conv_dgrad_tiles_m(N, H, W, C, Co, tile)
    part = torch.empty((T, C), dtype=torch.float32, device=dy.device)
    dz = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=dy.device)
    native.check(lib.ddpx_conv_dgrad_act(dy.data_ptr(), wd.data_ptr(), dz.data_ptr(), N, H, W, C, Co, tile,
                                         act.data_ptr(), part.data_ptr(), native.stream_handle()), "ddpx_conv_dgrad_act")
    return dz, (part, T)


def colsum_finish(part, T, C, out=None, accumulate=False, sgd=None):
    """out (=|+=) Σ_t part[t] in row-tile order, or applied as ``sgd``'s update (fused optimizer)."""
    _req(out is not None or sgd is not None, "colsum_finish: out or sgd")
    if out is not None:
        _req(out.numel() == C and out.is_contiguous() and out.dtype in (torch.float32, torch.bfloat16),
             "colsum_finish: bad out")
    lib = native.kernels()
    ws = torch.empty(lib.ddpx_colsum_ws_floats(T, C), dtype=torch.float32, device=part.device)
    native.check(lib.ddpx_colsum_finish(part.data_ptr(), T, C, ws.data_ptr(), native.ptr(out),
                                                     int(out is not None and out.dtype == torch.bfloat16),
                                                     int(accumulate), *native.sgd_args(sgd), native.stream_handle()),
                 "ddpx_colsum_finish")


def conv_dgrad(dy, wd, N, H, W, C, Co, tile=-1):
    """dx [N,H,W,C] bf16 = dgrad(dy [N*H*W, Co], wd [9,Co,C])."""
    _nhwc(dy, "dy", Co)
    _req(wd.numel() == 9 * Co * C, "conv_dgrad: bad weight buffer")
    dx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
    native.check(native.kernels().ddpx_conv_dgrad(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, C, Co, tile,
                                                  native.stream_handle()), "ddpx_conv_dgrad")
    return dx


def conv_dgrad_bn(dy, wd, N, H, W, C, Co, bn_y, a, b, mean, rstd, pool, tile=-1):
    """(dx, (part, B)): the data gradient of the conv, with the BatchNorm backward pass-1 sums of the block below
    (its pre-BN activation ``bn_y`` [N, H', W', C], H' = 2H when a 2x2 max-pool sits between) from the GEMM
    epilogue: ``bn_backward(..., part=(part, B))`` then skips its own reduce over dx and bn_y.  (dx, None) for
    the layers whose data-gradient tile has no fused variant (measured slower there, profiles/r5_vgg)."""
    _nhwc(dy, "dy", Co)
    _req(wd.numel() == 9 * Co * C, "conv_dgrad_bn: bad weight buffer")
    lib = native.kernels()
    B = lib.ddpx_conv_dgrad_parts(N, H, W, C, Co, tile)
    if B == 0:  # no fused variant for this layer's tile: plain data gradient, bn_backward reduces itself
        return conv_dgrad(dy, wd, N, H, W, C, Co, tile), None
    part = torch.empty((B, 2, C), dtype=torch.float32, device=dy.device)
    dx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
    native.check(lib.ddpx_conv_dgrad_bn(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, C, Co, tile,
                                        bn_y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        int(pool), part.data_ptr(), native.stream_handle()), "ddpx_conv_dgrad_bn")
    return dx, (part, B)


def conv_wgrad(dy, x, Co, Cr, out=None, accumulate=False, sgd=None, tile=-1, prepared=None):
    """Weight gradient in torch layout [Co,Cr,3,3] (written to ``out`` or applied through ``sgd``).
    ``prepared`` = (wf, wd) with ``sgd``: the update also rewrites the bf16 GEMM layouts ``weight_prep`` makes
    (whose zero channel padding it keeps), so the next forward needs no weight_prep pass."""
    N, H, W, C = x.shape
    _nhwc(x, "x")
    _nhwc(dy, "dy", Co)
    lib = native.kernels()
    P = N * H * W
    S = lib.ddpx_conv_wgrad_splits(P, C, Co, tile)
    part = torch.empty((S, Co, 9 * C), dtype=torch.float32, device=x.device)
    s = native.stream_handle()
    native.check(lib.ddpx_conv_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), S, N, H, W, C, Co, tile, s),
                 "ddpx_conv_wgrad")
    if sgd is None:
        _req(out is not None and out.numel() == Co * Cr * 9 and out.is_contiguous(), "conv_wgrad: bad out")
        _req(prepared is None, "conv_wgrad: prepared layouts are written by the fused SGD only")
    wf, wd = prepared if prepared is not None else (None, None)
    if prepared is not None:
        _req(wf.numel() == Co * 9 * C and wd.numel() == Co * 9 * C and wf.dtype == wd.dtype == torch.bfloat16,
             "conv_wgrad: bad prepared-weight buffers")
    native.check(lib.ddpx_conv_wgrad_reduce(part.data_ptr(), S, Co, Cr, C, native.ptr(out),
                                            int(out is not None and out.dtype == torch.bfloat16), int(accumulate),
                                            *native.sgd_args(sgd), native.ptr(wf), native.ptr(wd), s),
                 "ddpx_conv_wgrad_reduce")


# ---------------------------------------------------------------- stride 2 (csrc/kernels/conv_igemm_s2.hip)
def s2_out_hw(H: int, W: int):
    """(Ho, Wo) of a stride-2 convolution, 3x3 / pad 1 or 1x1 / pad 0 (the same for both, odd sizes included)."""
    _req(H >= 1 and W >= 1, f"stride-2 convolution: H, W >= 1 required, got {H}x{W}")
    return (H + 1) // 2, (W + 1) // 2


def _s2_shape(what, N, H, W, C, Co):
    _req(N >= 1 and C >= 8 and C % 8 == 0 and Co >= 8 and Co % 8 == 0,
         f"{what}: N >= 1 and channels in multiples of 8 required, got N={N} C={C} Co={Co}")
    return s2_out_hw(H, W)


def _s2_weight(w, name):
    _req(w.is_cuda and w.dtype == torch.bfloat16 and w.is_contiguous() and w.data_ptr() % 16 == 0,
         f"{name} must be contiguous 16-B aligned bf16 on GPU")


def _s2_fwd(what, ks, x, wf, Co, stats, tile):
    N, H, W, C = x.shape
    Ho, Wo = _s2_shape(what, N, H, W, C, Co)
    _req(wf.numel() == Co * ks * ks * C, f"{what}: weight/input channel mismatch")
    _nhwc(x, "x")
    _s2_weight(wf, "wf")
    lib = native.kernels()
    y = torch.empty((N * Ho * Wo, Co), dtype=torch.bfloat16, device=x.device)
    st, T, BM = None, 0, 0
    if stats:
        T = lib.ddpx_conv_s2_fwd_tiles_m(N, H, W, C, Co, ks, tile)
        BM = lib.ddpx_conv_s2_fwd_tile_rows(N, H, W, C, Co, ks, tile)
        native.check(min(T, BM, 0), what)
        st = torch.empty((T, 2, Co), dtype=torch.float32, device=x.device)
    native.check(lib.ddpx_conv_s2_fwd(x.data_ptr(), wf.data_ptr(), y.data_ptr(), native.ptr(st), N, H, W, C, Co, ks,
                                      tile, native.stream_handle()), what)
    return y, st, T, BM


def _s2_dgrad(what, ks, dy, wd, N, H, W, C, Co, tile):
    Ho, Wo = _s2_shape(what, N, H, W, C, Co)
    _req(wd.numel() == ks * ks * Co * C, f"{what}: bad weight buffer")
    _req(dy.numel() == N * Ho * Wo * Co, f"{what}: dy must be [N*Ho*Wo, Co]")
    _nhwc(dy, "dy", Co)
    _s2_weight(wd, "wd")
    dx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
    native.check(native.kernels().ddpx_conv_s2_dgrad(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, C, Co, ks,
                                                     tile, native.stream_handle()), what)
    return dx


def _s2_wgrad(what, ks, dy, x, Co, Cr, out, accumulate, sgd, tile):
    N, H, W, C = x.shape
    Ho, Wo = _s2_shape(what, N, H, W, C, Co)
    _req(1 <= Cr <= C, f"{what}: {Cr} real channels in {C} padded")
    _req(dy.numel() == N * Ho * Wo * Co, f"{what}: dy must be [N*Ho*Wo, Co]")
    _req((out is None) != (sgd is None), f"{what}: exactly one of out and sgd")
    if out is not None:
        _req(out.numel() == Co * Cr * ks * ks and out.is_contiguous()
             and out.dtype in (torch.float32, torch.bfloat16), f"{what}: bad out")
    _nhwc(x, "x")
    _nhwc(dy, "dy", Co)
    lib = native.kernels()
    S = lib.ddpx_conv_s2_wgrad_splits(N, H, W, C, Co, ks, tile)
    native.check(min(S, 0), what)
    part = torch.empty((S, Co, ks * ks * C), dtype=torch.float32, device=x.device)
    s = native.stream_handle()
    native.check(lib.ddpx_conv_s2_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), S, N, H, W, C, Co, ks, tile, s),
                 what)
    tail = (native.ptr(out), int(out is not None and out.dtype == torch.bfloat16), int(accumulate),
            *native.sgd_args(sgd))
    if ks == 3:
        native.check(lib.ddpx_conv_wgrad_reduce(part.data_ptr(), S, Co, Cr, C, *tail, None, None, s),
                     "ddpx_conv_wgrad_reduce")
    else:
        native.check(lib.ddpx_conv1x1_wgrad_reduce(part.data_ptr(), S, Co, Cr, C, *tail, s),
                     "ddpx_conv1x1_wgrad_reduce")


def conv_s2_fwd(x, wf, Co, stats=True, tile=-1):
    """3x3 / stride 2 / pad 1: y [N*Ho*Wo, Co] bf16 (+ per-tile BN statistics [T,2,Co] fp32 and tile rows),
    Ho = (H+1)//2, Wo = (W+1)//2.  ``wf`` [Co,9,C] from :func:`weight_prep`.  ``tile``: -1 default, 0 = 128x128,
    1 = 64x64."""
    return _s2_fwd("conv_s2_fwd", 3, x, wf, Co, stats, tile)


def conv_s2_dgrad(dy, wd, N, H, W, C, Co, tile=-1):
    """dx [N,H,W,C] bf16 of the 3x3 / stride 2 convolution: dy [N*Ho*Wo, Co], wd [9,Co,C]."""
    return _s2_dgrad("conv_s2_dgrad", 3, dy, wd, N, H, W, C, Co, tile)


def conv_s2_wgrad(dy, x, Co, Cr, out=None, accumulate=False, sgd=None, tile=-1):
    """Weight gradient of the 3x3 / stride 2 convolution in torch layout [Co,Cr,3,3] (written to ``out``, fp32 or
    bf16, or applied through ``sgd``)."""
    _s2_wgrad("conv_s2_wgrad", 3, dy, x, Co, Cr, out, accumulate, sgd, tile)


def weight_prep_1x1(w, wf, wd):
    """fp32 torch weight [Co,Ci,1,1] -> bf16 [Co,Cp], zero-padded channels.  The forward's ``wf`` and the data
    gradient's ``wd`` are the same array: pass one buffer twice, or two buffers to get two copies."""
    Co, Ci = w.shape[0], w.shape[1]
    Cp = padded_channels(Ci)
    _req(tuple(w.shape) == (Co, Ci, 1, 1) and w.dtype == torch.float32 and w.is_contiguous(), "bad 1x1 conv weight")
    _req(wf.numel() == Co * Cp and wd.numel() == Co * Cp and wf.dtype == wd.dtype == torch.bfloat16,
         "bad prepared-weight buffers")
    _req(w.is_cuda, "weight_prep_1x1: w must be on GPU")
    _s2_weight(wf, "wf")
    _s2_weight(wd, "wd")
    native.check(native.kernels().ddpx_conv1x1_weight_prep(w.data_ptr(), Co, Ci, Cp, wf.data_ptr(), wd.data_ptr(),
                                                           native.stream_handle()), "ddpx_conv1x1_weight_prep")


def conv1x1_s2_fwd(x, wf, Co, stats=True):
    """1x1 / stride 2 / pad 0 (the projection shortcut): y [N*Ho*Wo, Co] bf16 (+ BN statistics as
    :func:`conv_s2_fwd`).  ``wf`` [Co,C] from :func:`weight_prep_1x1`."""
    return _s2_fwd("conv1x1_s2_fwd", 1, x, wf, Co, stats, -1)


def conv1x1_s2_dgrad(dy, wd, N, H, W, C, Co):
    """dx [N,H,W,C] bf16 of the 1x1 / stride 2 convolution: dy . W at the even/even pixels, +0 elsewhere, all
    written by the one launch."""
    return _s2_dgrad("conv1x1_s2_dgrad", 1, dy, wd, N, H, W, C, Co, -1)


def conv1x1_s2_wgrad(dy, x, Co, Cr, out=None, accumulate=False, sgd=None):
    """Weight gradient of the 1x1 / stride 2 convolution in torch layout [Co,Cr,1,1]."""
    _s2_wgrad("conv1x1_s2_wgrad", 1, dy, x, Co, Cr, out, accumulate, sgd, -1)


# ---------------------------------------------------------------- 1x1 / stride 1 (csrc/kernels/conv1x1_s1.hip)
def _s1_shape(what, N, H, W, C, Co):
    _req(N >= 1 and H >= 1 and W >= 1 and C >= 8 and C % 8 == 0 and Co >= 8 and Co % 8 == 0,
         f"{what}: N, H, W >= 1 and channels in multiples of 8 required, got {N}x{H}x{W} C={C} Co={Co}")


def conv1x1_s1_fwd(x, wf, Co, stats=False):
    """1x1 / stride 1 / pad 0 (a Wide ResNet's stride-1 projection): (y [N*H*W, Co] bf16, None, 0, 0), the return
    shape of :func:`conv1x1_s2_fwd`.  ``wf`` [Co,C] from :func:`weight_prep_1x1`; the whole weight must fit a
    workgroup's LDS (Co * C * 2 B <= 64 KiB).  There is no BatchNorm-statistics epilogue: ``stats=True`` raises."""
    _req(not stats, "conv1x1_s1_fwd: no BatchNorm-statistics epilogue (the shortcut it serves has no BatchNorm)")
    N, H, W, C = x.shape
    _s1_shape("conv1x1_s1_fwd", N, H, W, C, Co)
    _req(wf.numel() == Co * C, "conv1x1_s1_fwd: weight/input channel mismatch")
    _nhwc(x, "x")
    _s2_weight(wf, "wf")
    y = torch.empty((N * H * W, Co), dtype=torch.bfloat16, device=x.device)
    native.check(native.kernels().ddpx_conv1x1_s1_fwd(x.data_ptr(), wf.data_ptr(), y.data_ptr(), N, H, W, C, Co,
                                                      native.stream_handle()), "conv1x1_s1_fwd")
    return y, None, 0, 0


def conv1x1_s1_dgrad(dy, wd, N, H, W, C, Co):
    """dx [N,H,W,C] bf16 = dy [N*H*W, Co] . wd [Co,C] of the 1x1 / stride 1 convolution."""
    _s1_shape("conv1x1_s1_dgrad", N, H, W, C, Co)
    _req(wd.numel() == Co * C, "conv1x1_s1_dgrad: bad weight buffer")
    _req(dy.numel() == N * H * W * Co, "conv1x1_s1_dgrad: dy must be [N*H*W, Co]")
    _nhwc(dy, "dy", Co)
    _s2_weight(wd, "wd")
    dx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
    native.check(native.kernels().ddpx_conv1x1_s1_dgrad(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, C, Co,
                                                        native.stream_handle()), "conv1x1_s1_dgrad")
    return dx


def conv1x1_s1_wgrad(dy, x, Co, Cr, out=None, accumulate=False, sgd=None):
    """Weight gradient of the 1x1 / stride 1 convolution in torch layout [Co,Cr,1,1]: written to ``out`` (fp32 or
    bf16, optionally accumulated) or applied through ``sgd``.  Per-slab partial sums reduced in slab order: the
    result is bitwise reproducible."""
    what = "conv1x1_s1_wgrad"
    N, H, W, C = x.shape
    _s1_shape(what, N, H, W, C, Co)
    _req(1 <= Cr <= C, f"{what}: {Cr} real channels in {C} padded")
    _req(dy.numel() == N * H * W * Co, f"{what}: dy must be [N*H*W, Co]")
    _req((out is None) != (sgd is None), f"{what}: exactly one of out and sgd")
    if out is not None:
        _req(out.numel() == Co * Cr and out.is_contiguous() and out.dtype in (torch.float32, torch.bfloat16),
             f"{what}: bad out")
    _nhwc(x, "x")
    _nhwc(dy, "dy", Co)
    lib = native.kernels()
    S = lib.ddpx_conv1x1_s1_wgrad_slabs(N, H, W, C, Co)
    native.check(min(S, 0), what)
    part = torch.empty((S, Co, C), dtype=torch.float32, device=x.device)
    s = native.stream_handle()
    native.check(lib.ddpx_conv1x1_s1_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), S, N, H, W, C, Co, s), what)
    native.check(lib.ddpx_conv1x1_wgrad_reduce(part.data_ptr(), S, Co, Cr, C, native.ptr(out),
                                               int(out is not None and out.dtype == torch.bfloat16), int(accumulate),
                                               *native.sgd_args(sgd), s), "ddpx_conv1x1_wgrad_reduce")


def bn_finalize(stats, T, BM, M, bn_mod, training, a, b, mean, rstd):
    C = bn_mod.num_features
    lib = native.kernels()
    nbt = bn_mod.num_batches_tracked if (training and bn_mod.num_batches_tracked is not None) else None
    native.check(lib.ddpx_bn_finalize(native.ptr(stats), T, BM, M, C, bn_mod.weight.data_ptr(),
                                      bn_mod.bias.data_ptr(), bn_mod.running_mean.data_ptr(),
                                      bn_mod.running_var.data_ptr(), native.ptr(nbt), float(bn_mod.momentum),
                                      float(bn_mod.eps), int(training), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), native.stream_handle()), "ddpx_bn_finalize")


def bn_finalize_sync(stats, T, BM, M, bn_mod, a, b, mean, rstd, comm):
    """SyncBatchNorm forward statistics (training): this rank's (mean, M2) from the tile statistics, one
    all-gather of [2][C] per rank on the current stream (RCCL: graph-capturable), then the rank-ordered
    Chan merge + running-stat update + affine coefficients in ``ddpx_bn_finalize``.  Every rank must hold
    the same number of rows M (equal DistributedSampler shards)."""
    C = bn_mod.num_features
    lib = native.kernels()
    dev = a.device
    local = torch.empty(2 * C, dtype=torch.float32, device=dev)
    native.check(lib.ddpx_bn_local_stats(stats.data_ptr(), T, BM, M, C, local.data_ptr(), native.stream_handle()),
                 "ddpx_bn_local_stats")
    ws = comm.world_size
    gathered = torch.empty(ws * 2 * C, dtype=torch.float32, device=dev)
    comm.allgather(gathered, local)
    bn_finalize(gathered, ws, M, ws * M, bn_mod, True, a, b, mean, rstd)


def _second_grad(gout, gout2, C, part):
    """Checks of the second gradient of a block below a residual block (``gout``'s shape; the kernels use
    gout + gout2 in fp32)."""
    if gout2 is None:
        return
    _nhwc(gout2, "gout2", C)
    _req(gout2.shape == gout.shape, f"gout2 {tuple(gout2.shape)} must have gout's shape {tuple(gout.shape)}")
    _req(part is None, "the data gradient's BatchNorm sums cover one gradient: part must be None with gout2")


def bn_backward_sync(gout, y, a, b, mean, rstd, N, H, W, C, pool, comm, dgamma=None, dbeta=None,
                     accumulate=False, part=None, gout2=None):
    """SyncBatchNorm backward: local (sum dy, sum dy*xhat) -> all-reduce -> dy with the global means;
    dgamma / dbeta stay local (DDP averages them, as torch's SyncBatchNorm).  ``part``: the local pass-1
    partials from the data gradient's epilogue (``conv_dgrad_bn``), as in ``bn_backward``.  ``gout2``: a second
    gradient of the block's output, as in ``bn_backward``."""
    _nhwc(gout, "gout", C)
    _nhwc(y, "y", C)
    _second_grad(gout, gout2, C, part)
    lib = native.kernels()
    dev = y.device
    sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
    gdt = dgamma.dtype if dgamma is not None else torch.float32
    s = native.stream_handle()
    if part is not None:
        pt, B = part
        native.check(lib.ddpx_bn_bwd_sums_from_part(pt.data_ptr(), B, C, sums.data_ptr(), native.ptr(dgamma),
                                                    native.ptr(dbeta), int(gdt == torch.bfloat16), int(accumulate),
                                                    s), "ddpx_bn_bwd_sums_from_part")
    else:
        B = lib.ddpx_bn_bwd_blocks(N, H, W, C)
        pt = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
        tail = (y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, H, W, C, int(pool), 1,
                pt.data_ptr(), sums.data_ptr(), native.ptr(dgamma), native.ptr(dbeta), int(gdt == torch.bfloat16),
                int(accumulate), s)
        if gout2 is not None:
            native.check(lib.ddpx_bn_bwd_sums_2g(gout.data_ptr(), gout2.data_ptr(), *tail), "ddpx_bn_bwd_sums_2g")
        else:
            native.check(lib.ddpx_bn_bwd_sums(gout.data_ptr(), *tail), "ddpx_bn_bwd_sums")
    comm.allreduce_(sums, op="sum")
    native.check(lib.ddpx_scale_f32(sums.data_ptr(), 2 * C, 1.0 / (comm.world_size * N * H * W), s), "ddpx_scale_f32")
    dy = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=dev)
    tail = (y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), sums.data_ptr(),
            sums[C:].data_ptr(), N, H, W, C, int(pool), 1, dy.data_ptr(), s)
    if gout2 is not None:
        native.check(lib.ddpx_bn_bwd_apply_2g(gout.data_ptr(), gout2.data_ptr(), *tail), "ddpx_bn_bwd_apply_2g")
    else:
        native.check(lib.ddpx_bn_bwd_apply(gout.data_ptr(), *tail), "ddpx_bn_bwd_apply")
    return dy


def bn_apply(y, a, b, N, H, W, C, relu=True, pool=False, res=None, out=None):
    """[maxpool2](relu(a*y + b)) [N, H', W', C] bf16.  ``res`` [N, H, W, C] bf16 (non-pooled only): the skip operand
    of a residual block, out = res + relu(a*y + b), added in fp32 and rounded once.  ``out``: the result's storage
    (any bf16 tensor of N*H'*W'*C contiguous elements)."""
    _nhwc(y, "y", C)
    _req(y.numel() == N * H * W * C, "bn_apply: y must hold N*H*W*C elements")
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=y.device)
    else:
        _nhwc(out, "out")
        _req(out.numel() == N * Ho * Wo * C, "bn_apply: out must hold N*H'*W'*C elements")
    if res is not None:
        _nhwc(res, "res", C)
        _req(res.numel() == N * H * W * C, "bn_apply: res must hold N*H*W*C elements")
        native.check(native.kernels().ddpx_bn_apply_res(y.data_ptr(), a.data_ptr(), b.data_ptr(), res.data_ptr(), N, H,
                                                        W, C, int(relu), int(pool), out.data_ptr(),
                                                        native.stream_handle()), "ddpx_bn_apply_res")
        return out
    native.check(native.kernels().ddpx_bn_apply(y.data_ptr(), a.data_ptr(), b.data_ptr(), N, H, W, C, int(relu),
                                                int(pool), out.data_ptr(), native.stream_handle()), "ddpx_bn_apply")
    return out


def bn_backward(gout, y, a, b, mean, rstd, N, H, W, C, pool, dgamma=None, dbeta=None, accumulate=False,
                sgd_gamma=None, sgd_beta=None, part=None, gout2=None, dy=None, gadd=None):
    """dy [N*H*W, C] bf16; dgamma/dbeta stored (fp32/bf16) or applied through sgd_gamma / sgd_beta.  ``part`` =
    (partials [B, 2, C], B): the pass-1 sums already made by the data gradient that produced ``gout``
    (``conv_dgrad_bn``).  ``gout2`` (``gout``'s shape, with ``part=None``): a second gradient of the block's output
    — the block below a residual block gets one from the branch and one from the skip; the kernels use
    gout + gout2 in fp32 and never store the sum.  ``dy``: the result's storage.  ``gadd`` ([N*H*W, C] bf16, not
    pooled, not with ``gout2``): added on the output side, dy = bf16(dx + gadd) rounded once — the gradient that the
    shortcut of a pre-activation residual block carries past this BatchNorm; the sums, dgamma and dbeta do not see
    it."""
    _nhwc(gout, "gout", C)
    _nhwc(y, "y", C)
    _second_grad(gout, gout2, C, part)
    if gadd is not None:
        _req(gout2 is None, "bn_backward: gadd does not combine with gout2 (a block below a projection has no gadd)")
        _req(not pool, "bn_backward: gadd needs a block without a pool")
        _nhwc(gadd, "gadd", C)
        _req(gadd.numel() == N * H * W * C, "bn_backward: gadd must hold N*H*W*C elements")
    ga = () if gadd is None else (gadd.data_ptr(),)
    sfx = "" if gadd is None else "_add"
    if dy is not None:
        _nhwc(dy, "dy")
        _req(dy.numel() == N * H * W * C, "bn_backward: dy must hold N*H*W*C elements")
    lib = native.kernels()
    dev = y.device
    if part is not None:
        pt, B = part
        c1 = torch.empty(C, dtype=torch.float32, device=dev)
        c2 = torch.empty(C, dtype=torch.float32, device=dev)
        if dy is None:
            dy = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=dev)
        gdt = dgamma.dtype if dgamma is not None else torch.float32
        sg, sb = native.sgd_args(sgd_gamma), native.sgd_args(sgd_beta)
        lr = sg[3] if sgd_gamma is not None else None
        mom, wd = (sg[4], sg[5]) if sgd_gamma is not None else (0.0, 0.0)
        fn = getattr(lib, "ddpx_bn_bwd_tail" + sfx)
        native.check(fn(gout.data_ptr(), *ga, y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                        rstd.data_ptr(), N, H, W, C, int(pool), 1, pt.data_ptr(), B, c1.data_ptr(), c2.data_ptr(),
                        native.ptr(dgamma), native.ptr(dbeta), int(gdt == torch.bfloat16), int(accumulate),
                        dy.data_ptr(), sg[0], sg[1], sb[0], sb[1], lr, mom, wd, native.stream_handle()),
                     "ddpx_bn_bwd_tail" + sfx)
        return dy
    B = lib.ddpx_bn_bwd_blocks(N, H, W, C)
    part = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
    c1 = torch.empty(C, dtype=torch.float32, device=dev)
    c2 = torch.empty(C, dtype=torch.float32, device=dev)
    if dy is None:
        dy = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=dev)
    gdt = dgamma.dtype if dgamma is not None else torch.float32
    sg, sb = native.sgd_args(sgd_gamma), native.sgd_args(sgd_beta)
    lr = sg[3] if sgd_gamma is not None else None
    mom, wd = (sg[4], sg[5]) if sgd_gamma is not None else (0.0, 0.0)
    tail = (y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, H, W, C, int(pool), 1,
            part.data_ptr(), c1.data_ptr(), c2.data_ptr(), native.ptr(dgamma), native.ptr(dbeta),
            int(gdt == torch.bfloat16), int(accumulate), dy.data_ptr(), sg[0], sg[1], sb[0], sb[1], lr, mom, wd,
            native.stream_handle())
    if gadd is not None:
        native.check(lib.ddpx_bn_bwd_add(gout.data_ptr(), gadd.data_ptr(), *tail), "ddpx_bn_bwd_add")
    elif gout2 is not None:
        native.check(lib.ddpx_bn_bwd_2g(gout.data_ptr(), gout2.data_ptr(), *tail), "ddpx_bn_bwd_2g")
    else:
        native.check(lib.ddpx_bn_bwd(gout.data_ptr(), *tail), "ddpx_bn_bwd")
    return dy


# ---------------------------------------------------------------- pre-activation blocks (csrc/kernels/bn_preact.hip)
def preact_add(y, s, N, H, W, C, stats=True, out=None, eval_ab=None):
    """z = bf16(y + s), the shortcut add of a pre-activation residual block (fp32 add, one rounding), y and s
    [N*H*W, C] bf16.  Training (``stats``): (z, st, T, BM) with st [T, 2, C] fp32 the per-row-tile (mean, M2) of the
    stored z, in the layout :func:`bn_finalize` reads from the convolution epilogue.  Eval (``eval_ab`` = (a, b), the
    next BatchNorm's coefficients): (z, act) with act [N, H, W, C] = bf16(relu(a*z + b)) from the same pass, as
    :func:`bn_apply` computes it from the stored z (pass ``stats=False``).  ``out``: z's storage; may be ``y``.
    ``C % 8 == 0``, ``8 <= C <= 512``, operands below 2 GiB."""
    _req(C % 8 == 0 and 8 <= C <= 512, f"preact_add: channels in multiples of 8 up to 512 required, got {C}")
    _req(N >= 1 and H >= 1 and W >= 1, f"preact_add: N, H, W >= 1 required, got {(N, H, W)}")
    _req(N * H * W * C * 2 < 2 ** 31, "preact_add: operands of 2 GiB or more are not supported")
    _req(bool(stats) != (eval_ab is not None), "preact_add: statistics (training) or eval_ab (evaluation), one of them")
    _nhwc(y, "y", C)
    _nhwc(s, "s", C)
    _req(y.numel() == s.numel() == N * H * W * C, "preact_add: y and s must hold N*H*W*C elements")
    z = out
    if z is None:
        z = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=y.device)
    else:
        _nhwc(z, "out", C)
        _req(z.numel() == y.numel(), "preact_add: out must hold N*H*W*C elements")
    lib = native.kernels()
    if eval_ab is not None:
        a, b = eval_ab
        for v in (a, b):
            _req(v.is_cuda and v.dtype == torch.float32 and v.numel() == C and v.is_contiguous(),
                 "preact_add: eval_ab are fp32 [C]")
        act = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=y.device)
        native.check(lib.ddpx_preact_add(y.data_ptr(), s.data_ptr(), z.data_ptr(), None, a.data_ptr(), b.data_ptr(),
                                         act.data_ptr(), N, H, W, C, native.stream_handle()), "ddpx_preact_add")
        return z, act
    T, BM = lib.ddpx_preact_add_tiles(N, H, W, C), lib.ddpx_preact_add_tile_rows(N, H, W, C)
    native.check(min(T, BM, 0), "ddpx_preact_add_tiles")
    st = torch.empty((T, 2, C), dtype=torch.float32, device=y.device)
    native.check(lib.ddpx_preact_add(y.data_ptr(), s.data_ptr(), z.data_ptr(), st.data_ptr(), None, None, None, N, H,
                                     W, C, native.stream_handle()), "ddpx_preact_add")
    return z, st, T, BM


# ---------------------------------------------------------------- the basic-block join (csrc/kernels/bn_join.hip)
def _join_operands(what, N, H, W, C, res, proj, stats):
    """Checks of the join's second operand; the nine kernel arguments (res, y2, a2, b2, mean2, rstd2 pointers; None
    where absent).  ``stats``: the backward, whose ``proj`` carries the shortcut BatchNorm's mean and rstd too."""
    _req(C % 8 == 0 and 8 <= C <= 512, f"{what}: channels in multiples of 8 up to 512 required, got {C}")
    _req((res is None) != (proj is None), f"{what}: exactly one of res and proj")
    if res is not None:
        _nhwc(res, "res", C)
        _req(res.numel() == N * H * W * C, f"{what}: res must hold N*H*W*C elements")
        return (res.data_ptr(), None, None, None, None, None)
    _req(len(proj) == (5 if stats else 3), f"{what}: proj = (y2, a2, b2{', mean2, rstd2' if stats else ''})")
    y2 = proj[0]
    _nhwc(y2, "y2", C)
    _req(y2.numel() == N * H * W * C, f"{what}: y2 must hold N*H*W*C elements")
    for v in proj[1:]:
        _req(v.is_cuda and v.dtype == torch.float32 and v.numel() == C and v.is_contiguous(),
             f"{what}: the shortcut BatchNorm's coefficients are fp32 [C]")
    return (None, y2.data_ptr(), *(v.data_ptr() for v in proj[1:]), *([None] * (5 - len(proj))))


def _pad_operands(what, N, H, W, C, res, proj, pad, gout2, gout2_sub):
    """Checks of the option-A shortcut ``pad`` = x [N, Hx, Wx, C/2] and of the strided second gradient ``gout2_sub``
    [N, (H+1)//2, (W+1)//2, C] (the ``ddpx_bn_join_pad*`` kernels); (Hx, Wx), 0 without ``pad``."""
    _req(C % 8 == 0 and 8 <= C <= 512, f"{what}: channels in multiples of 8 up to 512 required, got {C}")
    _req(proj is None, f"{what}: pad / gout2_sub do not combine with proj")
    _req((res is None) != (pad is None), f"{what}: exactly one of res, proj and pad")
    _req(gout2 is None or gout2_sub is None, f"{what}: gout2 and gout2_sub together")
    _req(N * H * W * C * 2 < 2 ** 31, f"{what}: operands of 2 GiB or more are not supported")
    if gout2_sub is not None:
        _nhwc(gout2_sub, "gout2_sub", C)
        _req(tuple(gout2_sub.shape) == (N, (H + 1) // 2, (W + 1) // 2, C),
             f"{what}: gout2_sub must be [N, (H+1)//2, (W+1)//2, C], got {tuple(gout2_sub.shape)}")
    if pad is None:
        _nhwc(res, "res", C)
        _req(res.numel() == N * H * W * C, f"{what}: res must hold N*H*W*C elements")
        return 0, 0
    _req(C % 32 == 0, f"{what}: the option-A shortcut needs C % 32 == 0, got {C}")
    _nhwc(pad, "pad", C // 2)
    _req(pad.dim() == 4 and pad.shape[0] == N and s2_out_hw(pad.shape[1], pad.shape[2]) == (H, W),
         f"{what}: pad {tuple(pad.shape)} is not the [N, Hx, Wx, C/2] input of a stride-2 block with output "
         f"{(N, H, W, C)}")
    _req(pad.numel() * 2 < 2 ** 31, f"{what}: operands of 2 GiB or more are not supported")
    return pad.shape[1], pad.shape[2]


def bn_join(y, a, b, N, H, W, C, res=None, proj=None, out=None, pad=None):
    """relu(a*y + b + s) [N, H, W, C] bf16, the join of a basic residual block: the ReLU after the add, fp32
    arithmetic, one rounding.  Exactly one of ``res`` ([N, H, W, C] bf16, the identity shortcut: s = res),
    ``proj`` = (y2, a2, b2) (the projection shortcut: s = a2*y2 + b2, y2 the raw output of the 1x1 / stride-2
    convolution, a2 / b2 its BatchNorm's coefficients from :func:`bn_finalize`) and ``pad`` = x [N, Hx, Wx, C/2]
    bf16 with (H, W) = ((Hx+1)//2, (Wx+1)//2) (the option-A shortcut: s = x[:, ::2, ::2] zero-padded by C/4 channels
    on each side, gathered inside the kernel; ``C % 32 == 0``)."""
    _nhwc(y, "y", C)
    _req(y.numel() == N * H * W * C, "bn_join: y must hold N*H*W*C elements")
    if pad is not None:
        Hx, Wx = _pad_operands("bn_join", N, H, W, C, res, proj, pad, None, None)
        if out is None:
            out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=y.device)
        else:
            _nhwc(out, "out")
            _req(out.numel() == N * H * W * C, "bn_join: out must hold N*H*W*C elements")
        native.check(native.kernels().ddpx_bn_join_pad(y.data_ptr(), a.data_ptr(), b.data_ptr(), pad.data_ptr(), N, H,
                                                       W, C, Hx, Wx, out.data_ptr(), native.stream_handle()),
                     "ddpx_bn_join_pad")
        return out
    ops = _join_operands("bn_join", N, H, W, C, res, proj, False)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=y.device)
    else:
        _nhwc(out, "out")
        _req(out.numel() == N * H * W * C, "bn_join: out must hold N*H*W*C elements")
    native.check(native.kernels().ddpx_bn_join(y.data_ptr(), a.data_ptr(), b.data_ptr(), *ops[:4], N, H, W, C,
                                               out.data_ptr(), native.stream_handle()), "ddpx_bn_join")
    return out


def bn_join_sums(gout, y, a, b, mean, rstd, N, H, W, C, res=None, proj=None, gout2=None, pad=None, gout2_sub=None):
    """Pass 1 of :func:`bn_join_backward`: (part [V, B, 2, C] fp32, B), V = 1 (identity and pad; rows sum m, sum
    m*xhat) or 2 (projection; view 1 holds sum m, sum m*xhat2), with m = (gout + gout2) * [z > 0].  One row pair per
    reduce block, combined in a fixed order, no atomics."""
    _nhwc(gout, "gout", C)
    _nhwc(y, "y", C)
    _req(gout.numel() == y.numel() == N * H * W * C, "bn_join_backward: gout and y must hold N*H*W*C elements")
    if gout2 is not None:
        _nhwc(gout2, "gout2", C)
        _req(gout2.numel() == gout.numel(), "bn_join_backward: gout2 must have gout's size")
    if pad is not None or gout2_sub is not None:
        Hx, Wx = _pad_operands("bn_join_backward", N, H, W, C, res, proj, pad, gout2, gout2_sub)
        lib = native.kernels()
        B = lib.ddpx_bn_join_pad_blocks(N, H, W, C)
        native.check(min(B, 0), "ddpx_bn_join_pad_blocks")
        part = torch.empty((1, B, 2, C), dtype=torch.float32, device=y.device)
        native.check(lib.ddpx_bn_join_pad_bwd_sums(gout.data_ptr(), native.ptr(gout2), native.ptr(gout2_sub),
                                                   y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), native.ptr(res), native.ptr(pad), N, H, W, C, Hx,
                                                   Wx, part.data_ptr(), native.stream_handle()),
                     "ddpx_bn_join_pad_bwd_sums")
        return part, B
    ops = _join_operands("bn_join_backward", N, H, W, C, res, proj, True)
    lib = native.kernels()
    B = lib.ddpx_bn_join_blocks(N, H, W, C)
    native.check(min(B, 0), "ddpx_bn_join_blocks")
    part = torch.empty((1 if proj is None else 2, B, 2, C), dtype=torch.float32, device=y.device)
    native.check(lib.ddpx_bn_join_bwd_sums(gout.data_ptr(), native.ptr(gout2), y.data_ptr(), a.data_ptr(),
                                           b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), *ops, N, H, W, C,
                                           part.data_ptr(), native.stream_handle()), "ddpx_bn_join_bwd_sums")
    return part, B


def bn_join_merge(part, B, C, M, dgamma=None, dbeta=None, accumulate=False, sgd_gamma=None, sgd_beta=None):
    """(c1, c2) = (S0 / M, S1 / M) of one view ``part`` [B, 2, C] of the join's pass-1 sums, by the BatchNorm
    backward's merge kernels; dbeta = S0 / dgamma = S1 stored (fp32 or bf16, = or +=) or applied through
    sgd_gamma / sgd_beta."""
    c1 = torch.empty(C, dtype=torch.float32, device=part.device)
    c2 = torch.empty_like(c1)
    gdt = dgamma.dtype if dgamma is not None else torch.float32
    sg, sb = native.sgd_args(sgd_gamma), native.sgd_args(sgd_beta)
    lr = sg[3] if sgd_gamma is not None else sb[3]
    mom, wd = (sg[4], sg[5]) if sgd_gamma is not None else (sb[4], sb[5])
    native.check(native.kernels().ddpx_bn_join_bwd_merge(part.data_ptr(), B, C, M, c1.data_ptr(), c2.data_ptr(),
                                                         native.ptr(dgamma), native.ptr(dbeta),
                                                         int(gdt == torch.bfloat16), int(accumulate), sg[0], sg[1],
                                                         sb[0], sb[1], lr, mom, wd, native.stream_handle()),
                 "ddpx_bn_join_bwd_merge")
    return c1, c2


def bn_join_apply(gout, y, a, b, mean, rstd, c1, c2, N, H, W, C, res=None, proj=None, c2b=None, gout2=None, pad=None,
                  gout2_sub=None):
    """Pass 2 of :func:`bn_join_backward`: (dy, gm) in identity mode, (dy, dy2) in projection mode (``c2b``: the
    shortcut BatchNorm's c2), each [N*H*W, C] bf16; (dy, gs) in pad mode, gs [N, H, W, C/2] bf16."""
    if pad is not None or gout2_sub is not None:
        Hx, Wx = _pad_operands("bn_join_backward", N, H, W, C, res, proj, pad, gout2, gout2_sub)
        _req(c2b is None, "bn_join_backward: c2b comes with proj")
        dy = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=y.device)
        aux = torch.empty_like(dy) if pad is None else torch.empty((N, H, W, C // 2), dtype=torch.bfloat16,
                                                                   device=y.device)
        native.check(native.kernels().ddpx_bn_join_pad_bwd_apply(
            gout.data_ptr(), native.ptr(gout2), native.ptr(gout2_sub), y.data_ptr(), a.data_ptr(), b.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), native.ptr(res), native.ptr(pad), c1.data_ptr(), c2.data_ptr(), N, H, W,
            C, Hx, Wx, dy.data_ptr(), aux.data_ptr(), native.stream_handle()), "ddpx_bn_join_pad_bwd_apply")
        return dy, aux
    ops = _join_operands("bn_join_backward", N, H, W, C, res, proj, True)
    _req((proj is None) == (c2b is None), "bn_join_backward: c2b comes with proj")
    dy = torch.empty((N * H * W, C), dtype=torch.bfloat16, device=y.device)
    aux = torch.empty_like(dy)
    native.check(native.kernels().ddpx_bn_join_bwd_apply(gout.data_ptr(), native.ptr(gout2), y.data_ptr(),
                                                         a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                         rstd.data_ptr(), *ops, c1.data_ptr(), c2.data_ptr(),
                                                         native.ptr(c2b), N, H, W, C, dy.data_ptr(), aux.data_ptr(),
                                                         native.stream_handle()), "ddpx_bn_join_bwd_apply")
    return dy, aux


def bn_join_backward(gout, y, a, b, mean, rstd, N, H, W, C, res=None, proj=None, gout2=None, dgamma=None, dbeta=None,
                     accumulate=False, sgd_gamma=None, sgd_beta=None, dgamma2=None, dbeta2=None, accumulate2=False,
                     sgd_gamma2=None, sgd_beta2=None, pad=None, gout2_sub=None):
    """Backward of :func:`bn_join` given the gradient ``gout`` (+ ``gout2``, summed in fp32 and never stored) of its
    output; the ReLU mask is recomputed from the operands.  Identity (``res``): (dy, gm), gm = bf16(m) the skip
    gradient.  Projection (``proj`` = (y2, a2, b2, mean2, rstd2)): (dy, dy2), dy2 the gradient at y2.  dgamma /
    dbeta / accumulate / sgd_gamma / sgd_beta as :func:`bn_backward`; the same arguments with a 2 for the shortcut
    BatchNorm (its dbeta equals the branch's).  Three passes: the sums, one merge per BatchNorm, the apply.

    Option A (``pad`` = x [N, Hx, Wx, C/2], the downsampling block's input): (dy, gs), gs [N, H, W, C/2] =
    bf16(m[..., C/4 : 3C/4]) the skip gradient at the even pixels of x, compact; the zero-inserted array is never
    formed.  ``gout2_sub`` (with ``res`` or ``pad``, instead of ``gout2``): such a gs from the block above, a second
    gradient that exists at even (h, w) only and is read there from gout2_sub[n, h/2, w/2]."""
    part, B = bn_join_sums(gout, y, a, b, mean, rstd, N, H, W, C, res, proj, gout2, pad, gout2_sub)
    M = N * H * W
    c2b = None
    if proj is not None:  # the shortcut BatchNorm first: grad-ready order is the reverse of the registration order
        _, c2b = bn_join_merge(part[1], B, C, M, dgamma2, dbeta2, accumulate2, sgd_gamma2, sgd_beta2)
    c1, c2 = bn_join_merge(part[0], B, C, M, dgamma, dbeta, accumulate, sgd_gamma, sgd_beta)
    return bn_join_apply(gout, y, a, b, mean, rstd, c1, c2, N, H, W, C, res, proj, c2b, gout2, pad, gout2_sub)


def avgpool(x):
    N, H, W, C = x.shape
    _nhwc(x, "x")
    out = torch.empty((N, C), dtype=torch.bfloat16, device=x.device)
    native.check(native.kernels().ddpx_avgpool(x.data_ptr(), N, H * W, C, out.data_ptr(), native.stream_handle()),
                 "ddpx_avgpool")
    return out


def avgpool_backward(g, N, H, W, C):
    _nhwc(g, "g", C)
    gx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=g.device)
    native.check(native.kernels().ddpx_avgpool_bwd(g.data_ptr(), N, H * W, C, gx.data_ptr(), native.stream_handle()),
                 "ddpx_avgpool_bwd")
    return gx


def pool_shape(x):
    """(N, S, C) of an [N, H, W, C] or [N, S, C] tensor."""
    _req(x.dim() in (3, 4), f"expected [N, H, W, C] or [N, S, C], got {tuple(x.shape)}")
    return x.shape[0], math.prod(x.shape[1:-1]), x.shape[-1]


def gmaxpool(x, scale=1.0):
    """[N, H, W, C] (or [N, S, C]) bf16 -> [N, C]: ``scale * max`` over the pixels (global max pool with a feature
    scale; the product is formed in fp32 and rounded once).  ``C % 8 == 0``."""
    _nhwc(x, "x")
    N, S, C = pool_shape(x)
    _req(C % 8 == 0 and S >= 1, f"gmaxpool: C % 8 == 0 and S >= 1 required, got S={S} C={C}")
    out = torch.empty((N, C), dtype=torch.bfloat16, device=x.device)
    native.check(native.kernels().ddpx_gmaxpool(x.data_ptr(), N, S, C, float(scale), out.data_ptr(),
                                                native.stream_handle()), "ddpx_gmaxpool")
    return out


def gmaxpool_backward(g, x, scale=1.0):
    """Gradient of :func:`gmaxpool` at the saved input ``x``: ``scale * g`` at the first maximum of each (n, c)
    column (lowest pixel index among equal maxima, torch's rule), +0 elsewhere.  No index tensor is stored."""
    _nhwc(x, "x")
    N, S, C = pool_shape(x)
    _req(C % 8 == 0 and S >= 1, f"gmaxpool_backward: C % 8 == 0 and S >= 1 required, got S={S} C={C}")
    _nhwc(g, "g", C)
    _req(tuple(g.shape) == (N, C), f"gmaxpool_backward: g must be [{N}, {C}], got {tuple(g.shape)}")
    gx = torch.empty_like(x)
    native.check(native.kernels().ddpx_gmaxpool_bwd(g.data_ptr(), x.data_ptr(), N, S, C, float(scale), gx.data_ptr(),
                                                    native.stream_handle()), "ddpx_gmaxpool_bwd")
    return gx
