"""The reference's fp32 recipe on native MI355X kernels (``--dtype fp32``): the operator wrappers.  The model graphs
built from them (VGG / ResNet-9, DeepNN, MLP) and their plans are in ``ops/f32_native.py``.

The reference's ``singlegpu.py`` builds the VGG in fp32 and reports "fp32 model has accuracy"; these operators run
that precision end to end on ``csrc/kernels/f32_gemm.hip``, ``f32_bn.hip`` and ``f32_head.hip`` instead of
torch/MIOpen: exact-f32 MFMA (``v_mfma_f32_16x16x4_f32``) GEMMs for Linear and the 3x3 convolutions
(implicit GEMM over NHWC, weight gradients split over N*H*W and reduced in fixed order; the stride-2 3x3 and 1x1
convolutions of ``csrc/kernels/f32_conv_s2.hip``, which no model uses yet), BatchNorm2d
statistics / apply+ReLU+MaxPool / backward, global average pool and the classifier head + cross-entropy
(``ddpx_f32_head_fwd`` / ``_fwd_soft`` / ``_bwd``, 1..128 classes).
"""
from __future__ import annotations

import os

import torch

from ..runtime import native
from .conv import pool_shape

DENSE_KC, DENSE_OC, IM2COL_KC, IM2COL_OC = 0, 1, 2, 3
F_RELU, F_ACCUM = 1, 2

_P, _I, _I64, _F = native.c_void_p, native.c_int, native.c_int64, native.c_float
for _sig in (
        ("ddpx_f32_gemm", _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I64, _P, _P, _I, _I,
         _P),
        ("ddpx_f32_splitk_reduce", _I, _P, _I, _I64, _P, _I, _P),
        ("ddpx_f32_conv_wprep", _I, _P, _I, _I, _I, _P, _P, _P),
        ("ddpx_f32_conv_wgrad_reduce", _I, _P, _I, _I, _I, _I, _P, _I, _P),
        ("ddpx_f32_bn_stats", _I, _P, _I, _I, _I, _P, _P),
        ("ddpx_f32_bn_finalize", _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _F, _F, _I, _P, _P, _P, _P, _P, _P),
        ("ddpx_f32_bn_apply", _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_bn_bwd_sums", _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_bias_act_bwd_sums", _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P),
        ("ddpx_f32_bn_bwd_finalize", _I, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P),
        ("ddpx_f32_bn_bwd_apply", _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P),
        # residual blocks: the skip operand of the apply, the second gradient of the backward (nullable pointers)
        ("ddpx_f32_bn_apply_res", _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_bn_bwd_sums_2g", _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_bn_bwd_apply_2g", _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_avgpool", _I, _P, _I, _I, _I, _P, _I, _P),
        ("ddpx_f32_gmaxpool", _I, _P, _I, _I, _I, _F, _P, _P),
        ("ddpx_f32_gmaxpool_bwd", _I, _P, _P, _I, _I, _I, _F, _P, _P),
        ("ddpx_f32_head_fwd", _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P),
        ("ddpx_f32_head_fwd_soft", _I, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _P, _P),
        ("ddpx_f32_head_bwd", _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _F, _P),
        ("ddpx_f32_nchw_flatten", _I, _P, _I, _I, _I, _I, _P, _P),
        ("ddpx_f32_set_staging", _I, _I),
        ("ddpx_f32_set_block", _I, _I),
        ("ddpx_f32_conv_fwd_stats", _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P),
        ("ddpx_dropout_fwd_f32", _I, _P, _P, _I64, _F, _P, _P, _P),
        ("ddpx_f32_colsum", _I, _P, _I, _I, _P, _I, _P),
        ("ddpx_f32_wgrad_sgd", _I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P),
        ("ddpx_f32_splitk_epi", _I, _P, _I, _I, _I, _P, _P, _P, _I, _P),
        ("ddpx_f32_wino_ok", _I, _I, _I, _I, _I),
        ("ddpx_f32_wino_conv_mask", _I, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P),
        ("ddpx_f32_colsum_part", _I, _P, _I, _I, _I, _P, _P),
        ("ddpx_f32_wino_wprep", _I, _P, _I, _I, _I, _P, _P, _P),
        ("ddpx_f32_wino_conv", _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P),
        ("ddpx_f32_wino_wgrad_ok", _I, _I, _I, _I, _I),
        ("ddpx_f32_wino_wgrad_splits", _I, _I, _I, _I, _I, _I),
        ("ddpx_f32_wino_wgrad", _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P),
):
    native.register_kernel_sig(*_sig)



def bn_chunk_rows(P: int, C: int) -> int:
    """Pixel rows per BatchNorm statistics chunk: ~16K elements, so a layer splits into enough workgroups
    to fill the chip (2048 at 64 channels x 32x32 x 512 images) with short per-thread row loops."""
    return max(8, min(P, 16384 // C))


def _req(c, msg):
    if not c:
        raise ValueError(msg)


def _f32(t, name):
    _req(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f"{name} must be contiguous fp32 on GPU")
    _req(t.data_ptr() % 16 == 0, f"{name} must be 16-B aligned")


def set_staging(dma: bool) -> bool:
    """GEMM operand staging of the f32 core: LDS-DMA ring (True, the default) or register-staged (False;
    DDPX_F32_STAGING=reg).  Returns the previous setting."""
    return bool(native.kernels().ddpx_f32_set_staging(int(bool(dma))))


def set_block(kb: int) -> int:
    """Summation block of the LDS-DMA core's blocked mode in 16-k K-steps (1 or 4 = default; anything else means
    4); 1 reproduces the register-staged kernel bitwise.  Returns the previous setting."""
    return int(native.kernels().ddpx_f32_set_block(int(kb)))


def _call(name, *args):
    native.check(getattr(native.kernels(), name)(*args, native.stream_handle()), name)


def gemm(amode, a, lda, bmode, b, ldb, M, N, K, out, ldc=None, bias=None, mask=None, relu=False, accumulate=False,
         geom=(0, 0, 0, 1), splits=1, split_stride=0, tile=-1):
    """out (+)= A B on the f32 MFMA core (operand modes: see f32_gemm.hip)."""
    flags = (F_RELU if relu else 0) | (F_ACCUM if accumulate else 0)
    _call("ddpx_f32_gemm", amode, a.data_ptr(), lda, bmode, b.data_ptr(), ldb, M, N, K, *geom, splits,
          out.data_ptr(), N if ldc is None else ldc, split_stride, native.ptr(bias), native.ptr(mask), flags, tile)


# ---------------------------------------------------------------------------------------------- Linear
# DDPX_F32_SPLITK (default 2): the batch-row (M <= 1024) Linear forward / data gradient as 2 in-grid K splits on
# 64x64 tiles (1024 workgroups instead of 512: 4 per CU) and one finishing pass with the epilogue
# (profiles/r5_mlp32: fc0 / fc1 152 / 178 -> 129 / 153 us + 7 us); 1 = one pass.  The split changes the summation
# into two half-length chains added at the end (closer to fp64, not bitwise the one-pass result).
_F32_SPLITK = int(os.environ.get("DDPX_F32_SPLITK", "2"))


def _splitk_linear(amode, a, lda, bmode, b, ldb, M, N, K, bias=None, mask=None, relu=False):
    S = _F32_SPLITK
    if S < 2 or M > 1024 or N % 4 or K < 1024 or (M * N) < (1 << 20):
        return None
    part = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
    gemm(amode, a, lda, bmode, b, ldb, M, N, K, part, tile=2, splits=S, split_stride=M * N)
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _call("ddpx_f32_splitk_epi", part.data_ptr(), S, M, N, out.data_ptr(), native.ptr(bias), native.ptr(mask),
          int(relu))
    return out


def linear_fwd(x, w, bias=None, relu=False):
    """y = x W^T + b [relu] — x [M,K], W [N,K] (torch layout)."""
    M, K = x.shape
    N = w.shape[0]
    _f32(x, "x")
    _f32(w, "w")
    _req(w.shape[1] == K, "linear_fwd: shape mismatch")
    y = _splitk_linear(DENSE_KC, x, K, DENSE_KC, w, K, M, N, K, bias=bias, relu=relu)
    if y is not None:
        return y
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    gemm(DENSE_KC, x, K, DENSE_KC, w, K, M, N, K, y, bias=bias, relu=relu)
    return y


def linear_dgrad(dy, w, mask=None):
    """dx = dy W [* (mask > 0)] — dy [M,N], W [N,K]."""
    M, N = dy.shape
    K = w.shape[1]
    _f32(dy, "dy")
    dx = _splitk_linear(DENSE_KC, dy, N, DENSE_OC, w, K, M, K, N, mask=mask)
    if dx is not None:
        return dx
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    gemm(DENSE_KC, dy, N, DENSE_OC, w, K, M, K, N, dx, mask=mask)
    return dx


def linear_wgrad(dy, x, out, accumulate=False):
    """dW (+)= dy^T x — dy [M,N], x [M,K], dW [N,K]."""
    M, N = dy.shape
    K = x.shape[1]
    _req(out.shape == (N, K) and out.is_contiguous(), "linear_wgrad: bad output")
    gemm(DENSE_OC, dy, N, DENSE_OC, x, K, N, K, M, out, accumulate=accumulate)


def linear_wgrad_sgd(dy, x, sgd):
    """W -= SGD(dy^T x) in the weight-gradient GEMM's epilogue (fused optimizer, single process); ``sgd`` =
    FlatParams.fused_spec(W).  False when the core cannot (register-staged core): the caller stores the
    gradient instead."""
    M, N = dy.shape
    K = x.shape[1]
    p, buf, sh, lr, mom, wd = sgd
    _req(p.numel() == N * K, "linear_wgrad_sgd: parameter size")
    r = native.kernels().ddpx_f32_wgrad_sgd(dy.data_ptr(), N, x.data_ptr(), K, M, N, K, -1, p.data_ptr(),
                                             native.ptr(buf), native.ptr(sh), lr.data_ptr(), float(mom), float(wd),
                                             native.stream_handle())
    if r == -6:
        return False
    native.check(r, "ddpx_f32_wgrad_sgd")
    return True


def colsum(x, out, accumulate=False):
    M, N = x.shape
    _call("ddpx_f32_colsum", x.data_ptr(), M, N, out.data_ptr(), int(accumulate))


HEAD_MAX_CLASSES = 128  # kWideNC of f32_head.hip


def head_forward(h, w, b, targets=None, soft=None):
    """(loss [scalar] or None, logits [M,NC], dlogits [M,NC] or None) of the fp32 classifier head.  ``soft``
    (:class:`ddpx.ops.loss.SoftTargets`, with ``targets``): loss and dlogits against the smoothed / mixed
    distribution."""
    M, K = h.shape
    NC = w.shape[0]
    _f32(h, "h")
    _req(1 <= NC <= HEAD_MAX_CLASSES, f"the fp32 head takes 1..{HEAD_MAX_CLASSES} classes, got {NC}")
    logits = torch.empty((M, NC), dtype=torch.float32, device=h.device)
    loss = dl = None
    if targets is not None:
        _req(targets.dtype == torch.int64 and targets.numel() == M, "targets must be int64 [M]")
        loss = torch.empty((), dtype=torch.float32, device=h.device)
        dl = torch.empty_like(logits)
    rows = None
    if NC > 16 and targets is not None:  # one wave per row there: the row losses, summed in row order
        rows = torch.empty((M,), dtype=torch.float32, device=h.device)
    tail = (M, K, NC, logits.data_ptr(), native.ptr(loss), native.ptr(dl), native.ptr(rows))
    if soft is not None and targets is not None:
        soft.check(M, h.device)
        _call("ddpx_f32_head_fwd_soft", h.data_ptr(), w.data_ptr(), b.data_ptr(), targets.data_ptr(),
              native.ptr(soft.tgt_b), native.ptr(soft.lam), soft.label_smoothing, *tail)
        return loss, logits, dl
    _call("ddpx_f32_head_fwd", h.data_ptr(), w.data_ptr(), b.data_ptr(), native.ptr(targets), *tail)
    return loss, logits, dl


def head_backward(dl, grad_out, h, w, dW, db, accumulate=False, relu_mask=False, want_dh=True, dh_scale=1.0):
    M, K = h.shape
    NC = w.shape[0]
    _req(1 <= NC <= HEAD_MAX_CLASSES, f"the fp32 head takes 1..{HEAD_MAX_CLASSES} classes, got {NC}")
    go = grad_out.float().contiguous() if grad_out is not None else None
    dh = torch.empty_like(h) if want_dh else None
    _call("ddpx_f32_head_bwd", dl.data_ptr(), native.ptr(go), h.data_ptr(), w.data_ptr(), M, K, NC, native.ptr(dW),
          native.ptr(db), int(accumulate), native.ptr(dh), int(relu_mask), float(dh_scale))
    return dh


def nchw_flatten(x):
    """torch.flatten(x, 1) of the NCHW tensor an NHWC fp32 activation [N,H,W,C] stands for: [N, C*H*W]."""
    N, H, W, C = x.shape
    _f32(x, "x")
    out = torch.empty((N, C * H * W), dtype=torch.float32, device=x.device)
    _call("ddpx_f32_nchw_flatten", x.data_ptr(), N, H * W, C, 0, out.data_ptr())
    return out


def nchw_unflatten(g, N, H, W, C):
    """Gradient of nchw_flatten: [N, C*H*W] -> NHWC [N,H,W,C]."""
    _f32(g, "g")
    out = torch.empty((N, H, W, C), dtype=torch.float32, device=g.device)
    _call("ddpx_f32_nchw_flatten", g.data_ptr(), N, H * W, C, 1, out.data_ptr())
    return out


def dropout_(x, p, rng, rng_done):
    """Inverted Dropout(p) of an fp32 tensor; generator state (seed, offset) device-resident in ``rng``."""
    _f32(x, "x")
    _req(x.numel() % 4 == 0, "dropout: numel % 4 != 0")
    out = torch.empty_like(x)
    _call("ddpx_dropout_fwd_f32", x.data_ptr(), out.data_ptr(), x.numel(), float(p), rng.data_ptr(),
          rng_done.data_ptr())
    return out


# ---------------------------------------------------------------------------------------------- conv / BN
def conv_channels(ci: int) -> int:
    """Input channels as stored (NHWC, 16-B pixels: the 3-channel image is zero-padded to 4)."""
    return max(4, (ci + 3) // 4 * 4)


def conv_wprep(w, wf, wd):
    Co, Ci = w.shape[:2]
    Cp = conv_channels(Ci)
    _req(wf.numel() == 9 * Cp * Co and (wd is None or wd.numel() == 9 * Co * Ci), "conv_wprep: bad buffers")
    _call("ddpx_f32_conv_wprep", w.data_ptr(), Co, Ci, Cp, wf.data_ptr(), native.ptr(wd))


def conv_fwd(x, wf, Co):
    """y [N*H*W, Co] = conv3x3(x [N,H,W,Cp], pad 1)."""
    N, H, W, C = x.shape
    _f32(x, "x")
    P = N * H * W
    y = torch.empty((P, Co), dtype=torch.float32, device=x.device)
    gemm(IM2COL_KC, x, 0, DENSE_OC, wf, Co, P, Co, 9 * C, y, geom=(C, H, W, 1))
    return y


def conv_fwd_stats(x, wf, Co):
    """(y, (stats, T, R)) — the forward convolution with the BatchNorm tile statistics (mean, M2 of every R-row
    output tile) emitted by the GEMM epilogue (LDS-DMA core), or (y, None) when that path does not apply."""
    N, H, W, C = x.shape
    _f32(x, "x")
    P = N * H * W
    y = torch.empty((P, Co), dtype=torch.float32, device=x.device)
    T = (P + 63) // 64  # enough rows of statistics for the smaller tile
    stats = torch.empty((T, 2, Co), dtype=torch.float32, device=x.device)
    r = native.kernels().ddpx_f32_conv_fwd_stats(x.data_ptr(), wf.data_ptr(), y.data_ptr(), N, H, W, C, Co,
                                                 stats.data_ptr(), native.stream_handle())
    if r < 0:
        if r == -10:  # register-staged core selected: plain forward, statistics by their own pass
            gemm(IM2COL_KC, x, 0, DENSE_OC, wf, Co, P, Co, 9 * C, y, geom=(C, H, W, 1))
            return y, None
        native.check(r, "ddpx_f32_conv_fwd_stats")
    return y, (stats, (P + r - 1) // r, r)


def conv_dgrad(dy, wd, N, H, W, C, Co):
    """dx [N,H,W,C] = transposed conv of dy [N*H*W, Co] with wd [(r,s,co), ci]."""
    _f32(dy, "dy")
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
    gemm(IM2COL_KC, dy, 0, DENSE_OC, wd, C, N * H * W, C, 9 * Co, dx, geom=(Co, H, W, -1))
    return dx


# ------------------------------------------------------------------ stride 2 (csrc/kernels/f32_conv_s2.hip)
# 3x3 / pad 1 and 1x1 / pad 0 at stride 2, the fp32 twins of ddpx.ops.conv's bf16 family: NHWC fp32, Ho = (H+1)//2,
# Wo = (W+1)//2, y / dy [N*Ho*Wo, Co].  ``tile``: -1 default, 0 = 128x128, 1 = 64x64.  Every check that needs no
# library comes first, so bad arguments raise ValueError without loading it.
def _s2_t(t, name, numel):
    _req(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f"{name} must be contiguous fp32 on GPU")
    _req(t.data_ptr() % 16 == 0, f"{name} must be 16-B aligned")
    _req(t.numel() == numel, f"{name} must hold {numel} elements, got {t.numel()}")


def _s2_shape(what, ks, N, H, W, C, Co):
    _req(ks in (1, 3), f"{what}: kernel size 1 or 3")
    _req(N >= 1 and H >= 1 and W >= 1, f"{what}: N, H, W >= 1 required, got {N}x{H}x{W}")
    _req(C >= 4 and C % 4 == 0 and Co >= 4 and Co % 4 == 0,
         f"{what}: channels in multiples of 4 required, got C={C} Co={Co}")
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    _req(max(N * H * W * C, N * Ho * Wo * Co, ks * ks * C * Co) * 4 < 2 ** 31, f"{what}: an operand of 2 GiB or more")
    return Ho, Wo


def _s2_fwd(what, ks, x, wf, Co, stats, tile):
    _req(x.dim() == 4, f"{what}: x must be [N,H,W,C]")
    N, H, W, C = x.shape
    Ho, Wo = _s2_shape(what, ks, N, H, W, C, Co)
    _s2_t(x, "x", N * H * W * C)
    _s2_t(wf, "wf", ks * ks * C * Co)
    lib = native.kernels()
    y = torch.empty((N * Ho * Wo, Co), dtype=torch.float32, device=x.device)
    st = None
    if stats:
        T = lib.ddpx_f32_conv_s2_fwd_tiles_m(N, H, W, C, Co, ks, tile)
        R = lib.ddpx_f32_conv_s2_fwd_tile_rows(N, H, W, C, Co, ks, tile)
        native.check(min(T, R, 0), what)
        st = (torch.empty((T, 2, Co), dtype=torch.float32, device=x.device), T, R)
    native.check(lib.ddpx_f32_conv_s2_fwd(x.data_ptr(), wf.data_ptr(), y.data_ptr(), native.ptr(st and st[0]), N, H, W,
                                          C, Co, ks, tile, native.stream_handle()), what)
    return y, st


def _s2_dgrad(what, ks, dy, wd, N, H, W, C, Co, tile):
    Ho, Wo = _s2_shape(what, ks, N, H, W, C, Co)
    _s2_t(dy, "dy", N * Ho * Wo * Co)
    _s2_t(wd, "wd", ks * ks * Co * C)
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
    native.check(native.kernels().ddpx_f32_conv_s2_dgrad(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, C, Co,
                                                         ks, tile, native.stream_handle()), what)
    return dx


def _s2_wgrad(what, ks, dy, x, Co, Ci, out, accumulate, tile):
    _req(x.dim() == 4, f"{what}: x must be [N,H,W,C]")
    N, H, W, C = x.shape
    Ho, Wo = _s2_shape(what, ks, N, H, W, C, Co)
    _req(1 <= Ci <= C and (ks == 3 or Ci == C), f"{what}: {Ci} real channels in {C} stored")
    _s2_t(x, "x", N * H * W * C)
    _s2_t(dy, "dy", N * Ho * Wo * Co)
    _s2_t(out, "out", Co * Ci * ks * ks)
    lib = native.kernels()
    S = lib.ddpx_f32_conv_s2_wgrad_splits(N, H, W, C, Co, ks, tile)
    native.check(min(S, 0), what)
    part = torch.empty((S, Co, ks * ks * C), dtype=torch.float32, device=x.device)
    native.check(lib.ddpx_f32_conv_s2_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), S, N, H, W, C, Co, ks, tile,
                                            native.stream_handle()), what)
    if ks == 3:  # slabs [S][Co][9*C] -> torch's [Co][Ci][3][3]
        _call("ddpx_f32_conv_wgrad_reduce", part.data_ptr(), S, Co, Ci, C, out.data_ptr(), int(accumulate))
    else:  # slabs [S][Co][C] with C == Ci: already torch's layout
        _call("ddpx_f32_splitk_reduce", part.data_ptr(), S, Co * C, out.data_ptr(), int(accumulate))


def conv_s2_fwd(x, wf, Co, stats=True, tile=-1):
    """3x3 / stride 2 / pad 1: (y [N*Ho*Wo, Co], (st, T, R)) with the BatchNorm tile statistics ``st`` [T,2,Co] of
    every R-row output tile for ``bn_forward(..., stats=)``, or (y, None).  ``wf`` [9*C, Co] from
    :func:`conv_wprep`."""
    return _s2_fwd("conv_s2_fwd", 3, x, wf, Co, stats, tile)


def conv_s2_dgrad(dy, wd, N, H, W, C, Co, tile=-1):
    """dx [N,H,W,C] of the 3x3 / stride 2 convolution: dy [N*Ho*Wo, Co], ``wd`` [9, Co, C] from
    :func:`conv_wprep`.  Four dense GEMMs over the parity classes of the input pixels, one launch."""
    return _s2_dgrad("conv_s2_dgrad", 3, dy, wd, N, H, W, C, Co, tile)


def conv_s2_wgrad(dy, x, Co, Ci, out, accumulate=False, tile=-1):
    """out [Co,Ci,3,3] (+)= the weight gradient of the 3x3 / stride 2 convolution from dy [N*Ho*Wo, Co] and
    x [N,H,W,Cp] (split over the output pixels, reduced in fixed order: bitwise reproducible)."""
    _s2_wgrad("conv_s2_wgrad", 3, dy, x, Co, Ci, out, accumulate, tile)


def conv1x1_wprep(w, wf):
    """torch's 1x1 weight [Co,Ci,1,1] -> ``wf`` [C, Co] (C = ``conv_channels(Ci)``, zero-padded), the forward's
    operand.  The data gradient reads ``w`` itself."""
    _req(w.dim() == 4 and tuple(w.shape[2:]) == (1, 1), "conv1x1_wprep: w must be [Co,Ci,1,1]")
    Co, Ci = w.shape[:2]
    C = conv_channels(Ci)
    _req(Co >= 4 and Co % 4 == 0, f"conv1x1_wprep: Co % 4 == 0 required, got {Co}")
    _s2_t(w, "w", Co * Ci)
    _s2_t(wf, "wf", C * Co)
    _call("ddpx_f32_conv1x1_wprep", w.data_ptr(), Co, Ci, C, wf.data_ptr())


def conv1x1_s2_fwd(x, wf, Co, stats=True, tile=-1):
    """1x1 / stride 2 / pad 0 (the projection shortcut), as :func:`conv_s2_fwd`; ``wf`` from
    :func:`conv1x1_wprep`."""
    return _s2_fwd("conv1x1_s2_fwd", 1, x, wf, Co, stats, tile)


def conv1x1_s2_dgrad(dy, w, N, H, W, C, Co, tile=-1):
    """dx [N,H,W,C] of the 1x1 / stride 2 convolution from torch's weight ``w`` [Co,C,1,1]: dy . W at the even /
    even pixels, +0 elsewhere, all written by the one launch."""
    _req(tuple(w.shape) == (Co, C, 1, 1), f"conv1x1_s2_dgrad: w must be [{Co},{C},1,1] (Ci == C)")
    return _s2_dgrad("conv1x1_s2_dgrad", 1, dy, w, N, H, W, C, Co, tile)


def conv1x1_s2_wgrad(dy, x, Co, Ci, out, accumulate=False, tile=-1):
    """out [Co,Ci,1,1] (+)= the weight gradient of the 1x1 / stride 2 convolution; Ci == C."""
    _s2_wgrad("conv1x1_s2_wgrad", 1, dy, x, Co, Ci, out, accumulate, tile)


# ------------------------------------------------------------------ Winograd F(2x2, 3x3) (csrc/kernels/f32_wino.hip)
# The forward and data-gradient 3x3 convolutions with >= DDPX_F32_WINO_MIN_C input channels (default 16: every
# layer but the 3-channel image one) run as fp32 Winograd F(2,3), MIOpen's algorithm for the
# stock fp32 recipe, with 2.25x fewer multiplies than the exact implicit GEMM.  DDPX_F32_WINO=0: the direct
# implicit GEMM everywhere (the weight gradient always is).
_WINO = os.environ.get("DDPX_F32_WINO", "1") != "0"
_WINO_MIN_C = int(os.environ.get("DDPX_F32_WINO_MIN_C", "16"))


def wino_applies(H, W, C, K) -> bool:
    return _WINO and C >= _WINO_MIN_C and bool(native.kernels().ddpx_f32_wino_ok(H, W, C, K))


def wino_wprep(w, uf, ud):
    """uf [16][Cp][Co] (forward) and ud [16][Co][Ci] (data gradient, flipped kernel) = G g G^T of w [Co,Ci,3,3]."""
    Co, Ci = w.shape[:2]
    Cp = conv_channels(Ci)
    _req(uf is None or uf.numel() == 16 * Cp * Co, "wino_wprep: bad forward buffer")
    _req(ud is None or ud.numel() == 16 * Co * Ci, "wino_wprep: bad data-gradient buffer")
    _call("ddpx_f32_wino_wprep", w.data_ptr(), Co, Ci, Cp, native.ptr(uf), native.ptr(ud))


def wino_conv(x, u, K, stats=False, bias=None, relu=False, mask=None):
    """y [N*H*W, K] = [relu](conv3x3(x [N,H,W,C]) [+ bias]) through F(2,3) with u [16][C][K]; with ``stats``:
    (y, (part, T, 256)), the BatchNorm chunk statistics of every 256-pixel output chunk from the epilogue.
    ``mask`` [N*H*W, K] (a data gradient through the ReLU of the block below): y = 0 where mask <= 0."""
    N, H, W, C = x.shape
    _f32(x, "x")
    if mask is not None:
        _f32(mask, "mask")
        _req(mask.numel() == N * H * W * K, "wino_conv: bad mask")
    y = torch.empty((N * H * W, K), dtype=torch.float32, device=x.device)
    T = (N * (H // 2) * (W // 2) + 63) // 64
    st = torch.empty((T, 2, K), dtype=torch.float32, device=x.device) if stats else None
    r = native.kernels().ddpx_f32_wino_conv_mask(x.data_ptr(), u.data_ptr(), y.data_ptr(), native.ptr(st),
                                                  native.ptr(bias), int(relu), native.ptr(mask), N, H, W, C, K,
                                                  native.stream_handle())
    native.check(r if r < 0 else 0, "ddpx_f32_wino_conv")
    return (y, (st, T, r)) if stats else y


def wgrad_splits(Co, Ncols, P):
    tiles = ((Co + 127) // 128) * ((Ncols + 127) // 128)
    s = max(1, min(P // 1024, (2048 + tiles - 1) // tiles))
    return s


# Weight gradient through F(2,3) too (csrc/kernels/f32_wino.hip wino_wgrad_kernel: dW = G^T (sum over tiles of
# (A dY A^T) (.) (B^T x B)) G, 4/9 of the direct product's multiplies); DDPX_F32_WINO_WGRAD=0: the direct split-K
# implicit GEMM.  Applies at Cp % 32 == 0, Co % 64 == 0, even H and W.
_WINO_WGRAD = os.environ.get("DDPX_F32_WINO_WGRAD", "1") != "0"
# DDPX_F32_WINO_WGRAD_PAD=0: 32-output-channel layers keep the direct weight gradient (A/B)
_WINO_WGRAD_PAD = os.environ.get("DDPX_F32_WINO_WGRAD_PAD", "1") != "0"


def wino_wgrad_applies(H, W, Cp, Co) -> bool:
    return _WINO and _WINO_WGRAD and bool(native.kernels().ddpx_f32_wino_wgrad_ok(H, W, Cp, Co))


def wino_wgrad(dy, x, Co, Ci, out, accumulate=False):
    """out [Co,Ci,3,3] (+)= the Winograd F(2,3) weight gradient from dy [P, Co] and x [N,H,W,Cp]."""
    N, H, W, Cp = x.shape
    _f32(x, "x")
    _req(dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == N * H * W * Co, "wino_wgrad: bad dy")
    _req(out.dtype == torch.float32 and out.is_contiguous() and out.numel() == Co * Ci * 9, "wino_wgrad: bad out")
    lib = native.kernels()
    S = lib.ddpx_f32_wino_wgrad_splits(N, H, W, Cp, Co)
    part = torch.empty((S, 16, Co, Cp), dtype=torch.float32, device=dy.device)
    du = torch.empty((16, Co, Cp), dtype=torch.float32, device=dy.device)
    _call("ddpx_f32_wino_wgrad", x.data_ptr(), dy.data_ptr(), part.data_ptr(), du.data_ptr(), N, H, W, Cp, Co, Ci, S,
          out.data_ptr(), int(accumulate))


def conv_wgrad(dy, x, Co, Ci, out, accumulate=False):
    """out [Co,Ci,3,3] (+)= weight gradient from dy [P, Co] and x [N,H,W,Cp]."""
    N, H, W, Cp = x.shape
    if wino_wgrad_applies(H, W, Cp, Co):
        return wino_wgrad(dy, x, Co, Ci, out, accumulate)
    if _WINO_WGRAD_PAD and Co == 32 and dy.is_cuda and wino_wgrad_applies(H, W, Cp, 64):
        # 32 output channels (DeepNN's 64 -> 32 layer): the Winograd weight gradient over dy zero-padded to 64
        # channels (its 4/9 multiplies beat the direct GEMM's tile padded from 32 to 64 rows: 121 us there)
        dyp = torch.nn.functional.pad(dy.view(-1, Co), (0, 64 - Co))
        tmp = torch.empty(64 * Ci * 9, dtype=torch.float32, device=dy.device)
        wino_wgrad(dyp, x, 64, Ci, tmp)
        o = out.view(-1)
        if accumulate:
            o.add_(tmp[:Co * Ci * 9])
        else:
            o.copy_(tmp[:Co * Ci * 9])
        return None
    return direct_wgrad(dy, x, Co, Ci, out, accumulate)


def direct_wgrad(dy, x, Co, Ci, out, accumulate=False):
    """conv_wgrad on the exact implicit GEMM (split over N*H*W, reduced in fixed order)."""
    N, H, W, Cp = x.shape
    P = N * H * W
    ncol = 9 * Cp
    S = wgrad_splits(Co, ncol, P)
    part = torch.empty((S, Co, ncol), dtype=torch.float32, device=dy.device)
    gemm(DENSE_OC, dy, Co, IM2COL_OC, x, 0, Co, ncol, P, part, geom=(Cp, H, W, 1), splits=S,
         split_stride=Co * ncol)
    _call("ddpx_f32_conv_wgrad_reduce", part.data_ptr(), S, Co, Ci, Cp, out.data_ptr(), int(accumulate))


def bn_forward(y, N, H, W, C, bn, training, pool, stats=None, comm=None, res=None, out=None):
    """(x_next, a, b, mean, rstd): statistics + running-stat update + [pool](relu(a*(y-mean)+b)), a = gamma*rstd,
    b = beta.  ``stats`` = (part, T, R): chunk statistics already made (the conv GEMM epilogue).  ``res``
    [N,H,W,C] (non-pooled only): the skip operand of a residual block, x_next = res + relu(...).  ``out``: x_next's
    storage (the element-exact tests place it in a guarded buffer).

    ``comm`` (SyncBatchNorm, ``--sync_bn`` under DDP; /root/reference/multigpu.py:127): this rank's (mean, M2) is
    merged from its chunk statistics (``ddpx_bn_local_stats``), all-gathered ([world][2][C], one collective on the
    current stream: graph-capturable on RCCL), and the finalize merges the ranks in rank order as equal chunks
    of P rows each, so the batch statistics and the running-stat update (unbiased with the global count, as
    torch's SyncBatchNorm) are the global ones.  Every rank holds the same P (equal DistributedSampler shards)."""
    dev = y.device
    P = N * H * W
    a = torch.empty(C, dtype=torch.float32, device=dev)
    b, mean, rstd = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    if training and stats is not None:
        part, T, R = stats
    else:
        R = bn_chunk_rows(P, C)
        T = (P + R - 1) // R
        part = torch.empty((T, 2, C), dtype=torch.float32, device=dev) if training else a
        if training:
            _call("ddpx_f32_bn_stats", y.data_ptr(), P, C, R, part.data_ptr())
    Ptot = P
    if training and comm is not None:
        local = torch.empty(2 * C, dtype=torch.float32, device=dev)
        native.check(native.kernels().ddpx_bn_local_stats(part.data_ptr(), T, R, P, C, local.data_ptr(),
                                                          native.stream_handle()), "ddpx_bn_local_stats")
        ws = comm.world_size
        part = torch.empty(ws * 2 * C, dtype=torch.float32, device=dev)
        comm.allgather(part, local)
        T, R, Ptot = ws, P, ws * P
    nbt = bn.num_batches_tracked if (training and bn.num_batches_tracked is not None) else None
    _call("ddpx_f32_bn_finalize", part.data_ptr(), T, R, Ptot, C, bn.weight.data_ptr(), bn.bias.data_ptr(),
          bn.running_mean.data_ptr(), bn.running_var.data_ptr(), native.ptr(nbt), float(bn.momentum),
          float(bn.eps), int(training), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
          native.ptr(_fin_ws(T, C, dev)))
    return bn_apply(y, a, b, mean, N, H, W, C, pool, res=res, out=out), a, b, mean, rstd


def bn_apply(y, a, b, mean, N, H, W, C, pool, res=None, out=None):
    """[maxpool2](relu(a*(y - mean) + b)) [N, H', W', C], plus ``res`` when given (``bn_forward``'s apply pass)."""
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=y.device)
    else:
        _f32(out, "out")
        _req(out.numel() == N * Ho * Wo * C, "bn_apply: out must hold N*H'*W'*C elements")
    if res is not None:
        _f32(res, "res")
        _req(res.numel() == N * H * W * C, "bn_apply: res must hold N*H*W*C elements")
        _call("ddpx_f32_bn_apply_res", y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), res.data_ptr(), N, H,
              W, C, 1, int(pool), out.data_ptr())
        return out
    _call("ddpx_f32_bn_apply", y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), N, H, W, C, 1, int(pool),
          out.data_ptr())
    return out


_FIN_SPLIT_MAX, _FIN_SPLIT_MAX_C = 32, 1024  # f32_bn.hip kFinSplitMax / kFinSplitMaxC


def _fin_ws(T, C, dev):
    """fp64 workspace [2][32][C] of the split BatchNorm merges (f32_bn.hip bn_fin_*), from the caching allocator
    on the current stream, or None where the merge does not split (the kernels then take the one-pass merge)."""
    if T < 1024 or C > _FIN_SPLIT_MAX_C:
        return None
    return torch.empty(2 * _FIN_SPLIT_MAX * C, dtype=torch.float64, device=dev)


def _chunk_part(P, C, dev):
    """(R, T, part): rows per chunk, chunk count, and the [T][2][C] buffer of a backward pass's per-chunk sums."""
    R = bn_chunk_rows(P, C)
    T = (P + R - 1) // R
    return R, T, torch.empty((T, 2, C), dtype=torch.float32, device=dev)


def _bwd_finalize(part, T, P, C, c1, c2, dgamma, dbeta, accumulate):
    """The fixed-order merge of ``part``: c1, c2 = its two column sums / P; dgamma (+)= second, dbeta (+)= first."""
    _call("ddpx_f32_bn_bwd_finalize", part.data_ptr(), T, P, C, c1.data_ptr(), c2.data_ptr(), native.ptr(dgamma),
          native.ptr(dbeta), int(accumulate), native.ptr(_fin_ws(T, C, part.device)))


def bn_backward(g, y, a, b, mean, rstd, N, H, W, C, pool, dgamma, dbeta, accumulate=False, comm=None, g2=None,
                dy=None):
    """dy [P, C] of BatchNorm+ReLU(+MaxPool) given the block output gradient g; dgamma/dbeta (+)= ...  ``g2``
    (``g``'s shape): a second gradient of the block's output — the block below a residual block gets one from the
    branch and one from the skip; the kernels use g + g2 and never store the sum.  ``dy``: the result's storage.

    ``comm`` (SyncBatchNorm): the per-channel means c1 = mean(dy), c2 = mean(dy * xhat) are summed over the ranks
    (one all-reduce of [2][C]) and divided by the world size — the global means, every rank holding P rows — before
    the apply; dgamma / dbeta stay this rank's sums (DDP averages them), as in torch's SyncBatchNorm."""
    _f32(g, "g")
    if g2 is not None:
        _f32(g2, "g2")
        _req(g2.shape == g.shape, f"g2 {tuple(g2.shape)} must have g's shape {tuple(g.shape)}")
    P = N * H * W
    R, T, part = _chunk_part(P, C, y.device)
    sums_tail = (y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, H, W, C, int(pool), R,
                 part.data_ptr())
    if g2 is not None:
        _call("ddpx_f32_bn_bwd_sums_2g", g.data_ptr(), g2.data_ptr(), *sums_tail)
    else:
        _call("ddpx_f32_bn_bwd_sums", g.data_ptr(), *sums_tail)
    cc = torch.empty(2 * C, dtype=torch.float32, device=y.device)
    c1, c2 = cc[:C], cc[C:]
    _bwd_finalize(part, T, P, C, c1, c2, dgamma, dbeta, accumulate)
    if comm is not None:
        comm.allreduce_(cc, op="sum")
        native.check(native.kernels().ddpx_scale_f32(cc.data_ptr(), 2 * C, 1.0 / comm.world_size,
                                                     native.stream_handle()), "ddpx_scale_f32")
    if dy is None:
        dy = torch.empty((P, C), dtype=torch.float32, device=y.device)
    else:
        _f32(dy, "dy")
        _req(dy.numel() == P * C, "bn_backward: dy must hold N*H*W*C elements")
    apply_tail = (y.data_ptr(), a.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), c1.data_ptr(),
                  c2.data_ptr(), N, H, W, C, int(pool), dy.data_ptr())
    if g2 is not None:
        _call("ddpx_f32_bn_bwd_apply_2g", g.data_ptr(), g2.data_ptr(), *apply_tail)
    else:
        _call("ddpx_f32_bn_bwd_apply", g.data_ptr(), *apply_tail)
    return dy


def avgpool(x):
    N, H, W, C = x.shape
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _call("ddpx_f32_avgpool", x.data_ptr(), N, H * W, C, out.data_ptr(), 0)
    return out


def avgpool_backward(g, N, H, W, C):
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=g.device)
    _call("ddpx_f32_avgpool", g.data_ptr(), N, H * W, C, dx.data_ptr(), 1)
    return dx


def gmaxpool(x, scale=1.0):
    """[N, H, W, C] (or [N, S, C]) fp32 -> [N, C]: ``scale * max`` over the pixels (global max pool with a feature
    scale).  ``C % 4 == 0``."""
    _f32(x, "x")
    N, S, C = pool_shape(x)
    _req(C % 4 == 0 and S >= 1, f"gmaxpool: C % 4 == 0 and S >= 1 required, got S={S} C={C}")
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _call("ddpx_f32_gmaxpool", x.data_ptr(), N, S, C, float(scale), out.data_ptr())
    return out


def gmaxpool_backward(g, x, scale=1.0):
    """Gradient of :func:`gmaxpool` at the saved input ``x``: ``scale * g`` at the first maximum of each (n, c)
    column (lowest pixel index among equal maxima, torch's rule), +0 elsewhere.  No index tensor is stored."""
    _f32(x, "x")
    _f32(g, "g")
    N, S, C = pool_shape(x)
    _req(C % 4 == 0 and S >= 1, f"gmaxpool_backward: C % 4 == 0 and S >= 1 required, got S={S} C={C}")
    _req(tuple(g.shape) == (N, C), f"gmaxpool_backward: g must be [{N}, {C}], got {tuple(g.shape)}")
    dx = torch.empty_like(x)
    _call("ddpx_f32_gmaxpool_bwd", g.data_ptr(), x.data_ptr(), N, S, C, float(scale), dx.data_ptr())
    return dx


# ------------------------------------------------------------------------- conv + bias + ReLU blocks (DeepNN)
def bias_act_backward(g, y, N, H, W, C, pool, plan, dbias, accumulate=False):
    """dy [P, C] and dbias (+)= sum dy of out = [maxpool2](y), y = relu(conv + bias) (the ReLU mask and the pool's
    first-max routing recomputed from y)."""
    _f32(g, "g")
    P = N * H * W
    one, zero = plan.ones[:C], plan.zeros[:C]
    R, T, part = _chunk_part(P, C, y.device)
    dy = torch.empty((P, C), dtype=torch.float32, device=y.device)
    # the sums pass writes dy = gz too where the 4-channel path applies (no sums needed for it: no normalisation)
    wrote = native.kernels().ddpx_f32_bias_act_bwd_sums(g.data_ptr(), y.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                                        N, H, W, C, int(pool), R, part.data_ptr(), dy.data_ptr(),
                                                        native.stream_handle())
    if wrote < 0:
        native.check(wrote, "ddpx_f32_bias_act_bwd_sums")
    _bwd_finalize(part, T, P, C, plan.scratch[:C], plan.scratch[C:2 * C], None, dbias, accumulate)
    if wrote != 1:
        _call("ddpx_f32_bn_bwd_apply", g.data_ptr(), y.data_ptr(), one.data_ptr(), zero.data_ptr(), zero.data_ptr(),
              one.data_ptr(), zero.data_ptr(), zero.data_ptr(), N, H, W, C, int(pool), dy.data_ptr())
    return dy


# DDPX_F32_DGRAD_MASK=1: the Winograd data gradient into a non-pooled conv + ReLU block applies that block's ReLU
# mask in its epilogue, and the block only sums the bias gradient (colsum_bias) instead of the one-pass
# bias_act_backward (default 0).  Measured even (profiles/r6_f32epi): the first conv's backward pass drops
# 156 -> 49 us, but the mask read in the 128 -> 64 layer's dgrad epilogue adds 126 us (377 -> 503).
_DGRAD_MASK = os.environ.get("DDPX_F32_DGRAD_MASK", "0") != "0"


def colsum_bias(dy, P, C, plan, dbias, accumulate=False):
    """dbias (+)= sum over the P rows of dy [P, C] (fixed-order chunk sums merged by bn_bwd_finalize)."""
    R, T, part = _chunk_part(P, C, dy.device)
    _call("ddpx_f32_colsum_part", dy.data_ptr(), P, C, R, part.data_ptr())
    _bwd_finalize(part, T, P, C, plan.scratch[:C], plan.scratch[C:2 * C], None, dbias, accumulate)
