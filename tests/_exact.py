"""Element-exact checking of the bf16 MFMA kernels (plain helper module, no fixtures).

The method: bf16 operands that are small integers make every product and every partial sum an integer
below 2**24, so an fp32 accumulator holds the exact result whatever the summation order, the tile, the
K split or MFMA's internal rounding.  A kernel must then equal a float64 reference element for element
(``torch.equal``: a signed zero passes, a NaN does not).

* operands: seeded integers, cast to bf16 (exact);
* :func:`require_exact` states the magnitude condition from the shapes, before any launch;
* :func:`poisoned`: operand storage with a leading dimension 8 larger than the logical inner extent, the
  padding filled with NaN: every legitimate 16-byte chunk ends inside the logical extent, so a NaN in the
  output is an overread;
* :func:`guarded`: the output as a view of a larger sentinel-filled buffer (extra columns, one extra row on
  each side); :func:`assert_guard` demands the sentinel's bits everywhere outside the view afterwards.

The float64 references (3x3 / pad 1 convolution and its two gradients; BatchNorm-affine + ReLU + 2x2 max-pool
with the "first maximum wins" routing) are plain torch code, themselves checked against ``F.conv2d`` and
CPU autograd by ``tests/test_exact_refs_cpu.py``.
"""
from __future__ import annotations

import functools

import torch

EXACT_LIMIT = 2 ** 24
SENTINEL = {torch.float32: 12345.0, torch.bfloat16: 3.0}

# ------------------------------------------------------------------ shapes (shared with the CPU self-test)
GEMM_KS = (8, 72, 904)
GEMM_AMAX = GEMM_BMAX = 4
CONV_XMAX, CONV_WMAX = 3, 2  # x and dy in [-3, 3], w in [-2, 2]

CONV_GEOMS = ((2, 1, 1), (3, 1, 8), (2, 2, 2), (1, 3, 5), (2, 5, 3), (3, 7, 7), (2, 12, 12), (5, 16, 16),
              (3, 20, 20), (1, 32, 32))
CONV_CHANNELS = ((3, 16), (8, 8), (16, 24), (24, 40), (64, 64), (64, 136), (128, 72))
# weight gradient only: 68 real channels in 72 padded (tail tile of 4 channels) and 72 (tail tile of 8)
WGRAD_CHANNELS = ((68, 24), (72, 24))
# geometries on which every tile config is run
CONV_CFG_GEOMS = ((2, 5, 3), (3, 7, 7), (5, 16, 16))
BN_SHAPES = ((2, 2, 2, 8), (3, 4, 6, 24), (4, 8, 8, 64))


def conv_pairs():
    """(geometry, channels) pairs of the default-tile tests: every geometry with two channel pairs, every
    channel pair on three geometries or more."""
    out = []
    nc = len(CONV_CHANNELS)
    for i, g in enumerate(CONV_GEOMS):
        out.append((g, CONV_CHANNELS[i % nc]))
        out.append((g, CONV_CHANNELS[(i + 3) % nc]))
    out.append((CONV_GEOMS[-1], CONV_CHANNELS[-1]))
    return out


def padded_channels(c):
    return max(8, (c + 7) // 8 * 8)


def require_exact(amax, bmax, k_total, what=""):
    """The condition under which fp32 accumulation of integer products is exact in any order."""
    assert amax * bmax * k_total < EXACT_LIMIT, f"{what}: {amax}*{bmax}*{k_total} is not below 2**24"


# ------------------------------------------------------------------ operands
def ints(shape, lo, hi, seed):
    """Seeded integers uniform in [lo, hi] as float64 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float64)


def choice(values, shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def mask_operand(shape, seed):
    """bf16 ReLU-mask operand with positive values, negative values, +0 and -0 (0x8000); (tensor, mask>0 as f64)."""
    vals = torch.tensor([1.0, 2.0, 0.5, -1.0, -3.0, 0.0, -0.0], dtype=torch.bfloat16)
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(seed)
    m = vals.repeat((n + 6) // 7)[:n][torch.randperm(n, generator=g)].reshape(tuple(shape))  # every value occurs
    bits = m.view(torch.int16)
    assert (bits == -32768).any() and (bits == 0).any() and (m > 0).any() and (m < 0).any()
    return m, (m > 0).to(torch.float64)


def poisoned(t, device):
    """2-D values -> bf16 view [R, C] of a device buffer [R, C + 8] whose padding columns hold NaN."""
    R, C = t.shape
    buf = torch.full((R, C + 8), float("nan"), dtype=torch.bfloat16, device=device)
    buf[:, :C] = t.to(torch.bfloat16).to(device)
    return buf[:, :C]


def guarded(M, N, dtype, device, ldc=None, c0=0):
    """(buffer [(M + 2), ldc], view [M, N] at row 1 / column c0), the buffer filled with the sentinel."""
    ldc = N + 8 if ldc is None else ldc
    assert ldc >= c0 + N
    buf = torch.full((M + 2, ldc), SENTINEL[dtype], dtype=dtype, device=device)
    return buf, buf[1:M + 1, c0:c0 + N]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_guard(buf, M, N, what, c0=0):
    """Every element of ``buf`` outside the view rows 1..M, columns c0..c0+N still holds the sentinel's bits."""
    want = _bits(torch.full((1,), SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device))
    bad = _bits(buf) != want
    bad[1:M + 1, c0:c0 + N] = False
    if bad.any():
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} guard elements overwritten, first at {idx} "
                             f"(buffer rows {buf.shape[0]}, ld {buf.shape[1]}, view [1:{M + 1}, {c0}:{c0 + N}])")


def assert_guard_1d(buf, lo, hi, what):
    want = _bits(torch.full((1,), SENTINEL[buf.dtype], dtype=buf.dtype, device=buf.device))
    bad = _bits(buf) != want
    bad[lo:hi] = False
    assert not bad.any(), f"{what}: {int(bad.sum())} guard words overwritten, first at {bad.nonzero()[:5].tolist()}"


def rounded(ref, dtype):
    """The float64 (integer-exact) reference as the kernel must store it: fp32, then RNE to bf16."""
    r = ref.to(torch.float32)
    return r.to(torch.bfloat16) if dtype == torch.bfloat16 else r


def assert_equal(got, want, what):
    """``torch.equal`` on values, with the count and the first mismatches on failure."""
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, \
        f"{what}: got {tuple(got.shape)} {got.dtype}, want {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return
    bad = ~(got == want)  # NaN compares unequal: counted
    idx = bad.nonzero()[:6]
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; (index, got, want): {first}")


# ------------------------------------------------------------------ float64 references: 3x3 / pad 1 / stride 1
def _pad_hw(t):
    return torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))  # NHWC: pad W and H by one


def conv_fwd_ref(x, w):
    """x [N,H,W,Ci], w [Co,Ci,3,3] (float64) -> y [N,H,W,Co]."""
    N, H, W, _ = x.shape
    xp = _pad_hw(x)
    y = torch.zeros((N, H, W, w.shape[0]), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return y


def conv_dgrad_ref(dy, w):
    """dy [N,H,W,Co], w [Co,Ci,3,3] -> dx [N,H,W,Ci]."""
    N, H, W, _ = dy.shape
    dxp = torch.zeros((N, H + 2, W + 2, w.shape[1]), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + H, kx:kx + W, :] += dy @ w[:, :, ky, kx]
    return dxp[:, 1:H + 1, 1:W + 1, :].contiguous()


def conv_wgrad_ref(dy, x):
    """dy [N,H,W,Co], x [N,H,W,Ci] -> dw [Co,Ci,3,3]."""
    N, H, W, Co = dy.shape
    Ci = x.shape[-1]
    xp = _pad_hw(x)
    dw = torch.zeros((Co, Ci, 3, 3), dtype=torch.float64)
    d2 = dy.reshape(-1, Co)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d2.t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
    return dw


@functools.lru_cache(maxsize=None)
def conv_case(geom, chans, seed=0):
    """Operands and float64 references of one convolution case, computed once and shared (treat as read-only):
    x [N,H,W,Ci], w [Co,Ci,3,3], dy [N,H,W,Co], bias [Co]; y, dx, dw."""
    N, H, W = geom
    Ci, Co = chans
    s = seed * 1000 + hash((geom, chans)) % 997
    x = ints((N, H, W, Ci), -CONV_XMAX, CONV_XMAX, s)
    w = ints((Co, Ci, 3, 3), -CONV_WMAX, CONV_WMAX, s + 1)
    dy = ints((N, H, W, Co), -CONV_XMAX, CONV_XMAX, s + 2)
    bias = ints((Co,), -8, 8, s + 3)
    return dict(x=x, w=w, dy=dy, bias=bias, y=conv_fwd_ref(x, w), dx=conv_dgrad_ref(dy, w),
                dw=conv_wgrad_ref(dy, x))


# ------------------------------------------------------------------ float64 reference: affine + ReLU [+ 2x2 max-pool]
def _windows(t):
    """[N,H,W,C] -> [N,H/2,W/2,C,4], the 2x2 window in scan order (q = 2*dh + dw)."""
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def _unwindows(t):
    N, Ho, Wo, C, _ = t.shape
    return t.reshape(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, C)


def bn_apply_ref(y, a, b, pool, relu=True):
    """relu(a*y + b), optionally 2x2 max-pooled.  y [N,H,W,C] float64, a / b [C]."""
    z = a * y + b
    r = z.clamp_min(0) if relu else z
    if not pool:
        return r
    return _windows(r).max(dim=-1).values


def route_ref(g, y, a, b, pool):
    """The gradient w.r.t. z = a*y + b of out = [pool](relu(z)) given g = d/d out: per window and channel the
    FIRST position in scan order with the strictly greatest relu(z) receives g; zeroed where z <= 0."""
    z = a * y + b
    if not pool:
        return torch.where(z > 0, g, torch.zeros_like(g))
    rw, zw = _windows(z.clamp_min(0)), _windows(z)
    best = torch.full(rw.shape[:-1], float("-inf"), dtype=torch.float64)
    arg = torch.zeros(rw.shape[:-1], dtype=torch.long)
    for q in range(4):
        upd = rw[..., q] > best
        best = torch.where(upd, rw[..., q], best)
        arg = torch.where(upd, torch.full_like(arg, q), arg)
    gz = torch.zeros_like(zw)
    for q in range(4):
        gz[..., q] = torch.where((arg == q) & (zw[..., q] > 0), g, torch.zeros_like(g))
    return _unwindows(gz)


def bn_backward_ref(g, y, a, b, mean, rstd, pool):
    """(dy, dgamma, dbeta, terms): dy = a*(gz - c1 - xhat*c2) with c1 = dbeta/M, c2 = dgamma/M; ``terms`` =
    |a|*(|gz| + |c1| + |xhat*c2|), the magnitude that scales dy's rounding bound."""
    gz = route_ref(g, y, a, b, pool)
    xhat = (y - mean) * rstd
    M = y.shape[0] * y.shape[1] * y.shape[2]
    dbeta = gz.sum((0, 1, 2))
    dgamma = (gz * xhat).sum((0, 1, 2))
    c1, c2 = dbeta / M, dgamma / M
    dy = a * (gz - c1 - xhat * c2)
    terms = a.abs() * (gz.abs() + c1.abs() + (xhat * c2).abs())
    return dy, dgamma, dbeta, terms


@functools.lru_cache(maxsize=None)
def bn_case(shape, pool, seed=0):
    """Inputs on which a*y + b, xhat and every product with g are exact and ties inside windows are frequent:
    y integers in [-8, 8], a from {-2, -1, -0.5, 0.5, 1, 2} (negative scales included), b / mean multiples of
    0.25 in [-2, 2], rstd from {0.5, 1, 2}, g integers in [-3, 3] (pooled size when ``pool``)."""
    N, H, W, C = shape
    s = seed * 1000 + hash((shape, pool)) % 997
    y = ints((N, H, W, C), -8, 8, s)
    a = choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (C,), s + 1)
    b = ints((C,), -8, 8, s + 2) * 0.25
    mean = ints((C,), -8, 8, s + 3) * 0.25
    rstd = choice([0.5, 1.0, 2.0], (C,), s + 4)
    g = ints((N, H // 2, W // 2, C) if pool else (N, H, W, C), -3, 3, s + 5)
    return dict(y=y, a=a, b=b, mean=mean, rstd=rstd, g=g)
