"""Element-exact tests of the 1x1 / stride-1 convolution (csrc/kernels/conv1x1_s1.hip): forward, data gradient and
slab-split weight gradient with integer operands (tests/_exact.py) against the float64 product of the same operands."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16

# (N, H, W, Ci, Co)
CASES = (
    (2, 5, 5, 16, 64),      # P = 50: a ragged last row tile
    (1, 9, 7, 8, 24),       # Co no multiple of 16, a half-empty K-step
    (1, 5, 5, 12, 16),      # 12 real channels in 16 padded, one column tile of 16 (the data gradient's shape)
    (3, 8, 8, 136, 72),     # three K blocks with a K tail; 15 weight-gradient tiles
    (3, 9, 9, 16, 64),      # P = 243: four weight-gradient slabs, the last one ragged
    (1, 6, 6, 16, 264),     # three sweeps of column tiles, the last tile 8 wide
    (2, 3, 3, 64, 128),     # weight gradient: two tiles per wave on the short staging list
    (1, 4, 4, 136, 136),    # weight gradient: 25 tiles, seven per wave
    (1, 4, 4, 128, 256),    # the LDS bound itself: a 64 KiB weight image, 32 weight-gradient tiles
    (1, 363, 363, 8, 8),   # 4118 row tiles: two per wave; 458 slabs
)


@functools.lru_cache(maxsize=None)
def _case(N, H, W, Ci, Co):
    """Operands (float64, CPU) and references, computed once (read-only): x [P,Ci], w [Co,Ci], dy [P,Co]."""
    P = N * H * W
    s = (((N * 512 + H) * 512 + W) * 512 + Ci) * 512 + Co
    x = X.ints((P, Ci), -X.CONV_XMAX, X.CONV_XMAX, s)
    w = X.ints((Co, Ci), -X.CONV_WMAX, X.CONV_WMAX, s + 1)
    dy = X.ints((P, Co), -X.CONV_XMAX, X.CONV_XMAX, s + 2)
    return dict(x=x, w=w, dy=dy, y=x @ w.t(), dx=dy @ w, dw=dy.t() @ x)


def _flanked(n, gpu):
    """(buffer, view of n bf16 elements at a 16-byte aligned offset) with NaN on both sides and inside."""
    buf = torch.full((n + 16,), float("nan"), dtype=BF16, device=gpu)
    return buf, buf[8:8 + n]


@pytest.mark.parametrize("shape", CASES, ids=lambda v: "x".join(map(str, v)))
def test_conv1x1_s1_exact(gpu, shape):
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    lib = native.kernels()
    N, H, W, Ci, Co = shape
    c = _case(*shape)
    Cp, P = X.padded_channels(Ci), N * H * W
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, Cp, "fwd")
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, Co, "dgrad")
    X.require_exact(X.CONV_XMAX, X.CONV_XMAX, P, "wgrad")
    tag = f"1x1/s1 {shape}"
    xn = F.pad(c["x"], (0, Cp - Ci)).to(BF16).to(gpu).reshape(N, H, W, Cp).contiguous()
    dy = c["dy"].to(BF16).to(gpu)
    wf = wd = torch.empty(Co * Cp, dtype=BF16, device=gpu)
    K.weight_prep_1x1(c["w"].reshape(Co, Ci, 1, 1).to(F32).to(gpu), wf, wd)
    s = native.stream_handle()

    # ---- forward and data gradient: the wrapper, then the C entry point on NaN-flanked storage
    want_y = X.rounded(c["y"], BF16)
    y, st, T, BM = K.conv1x1_s1_fwd(xn, wf, Co)
    assert st is None and (T, BM) == (0, 0)
    X.assert_equal(y, want_y, f"{tag} forward")
    buf, v = _flanked(P * Co, gpu)
    native.check(lib.ddpx_conv1x1_s1_fwd(xn.data_ptr(), wf.data_ptr(), v.data_ptr(), N, H, W, Cp, Co, s), "fwd")
    X.assert_equal(v.view(P, Co), want_y, f"{tag} forward on flanked storage")
    assert bool(torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + P * Co:]).all()), f"{tag} forward wrote outside y"

    want_dx = X.rounded(F.pad(c["dx"], (0, Cp - Ci)), BF16).reshape(N, H, W, Cp)
    X.assert_equal(K.conv1x1_s1_dgrad(dy, wd, N, H, W, Cp, Co), want_dx, f"{tag} dgrad")
    buf, v = _flanked(P * Cp, gpu)
    native.check(lib.ddpx_conv1x1_s1_dgrad(dy.data_ptr(), wd.data_ptr(), v.data_ptr(), N, H, W, Cp, Co, s), "dgrad")
    X.assert_equal(v.view(N, H, W, Cp), want_dx, f"{tag} dgrad on flanked storage")
    assert bool(torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + P * Cp:]).all()), f"{tag} dgrad wrote outside dx"

    # ---- weight gradient in torch layout: stored / accumulated, fp32 / bf16, bitwise reproducible, fused SGD
    S = lib.ddpx_conv1x1_s1_wgrad_slabs(N, H, W, Cp, Co)
    assert S >= 1
    if shape == (3, 9, 9, 16, 64):
        assert S >= 3 and P % 32 != 0
    nw = Co * Ci
    c0 = X.ints((Co, Ci), -8, 8, nw)
    for dt in (F32, BF16):
        for acc in (False, True):
            buf = torch.full((nw + 16,), X.SENTINEL[dt], dtype=dt, device=gpu)
            out = buf[8:8 + nw]
            if acc:
                out.copy_(c0.reshape(-1).to(dt))
            K.conv1x1_s1_wgrad(dy, xn, Co, Ci, out=out, accumulate=acc)
            what = f"{tag} wgrad {dt} accumulate {acc}"
            X.assert_equal(out.view(Co, Ci), X.rounded(c["dw"] + (c0 if acc else 0), dt), what)
            X.assert_guard_1d(buf, 8, 8 + nw, what)
    # the slabs themselves, behind a sentinel: nothing outside [S, Co, Cp] is written
    buf = torch.full((S * Co * Cp + 16,), X.SENTINEL[F32], dtype=F32, device=gpu)
    native.check(lib.ddpx_conv1x1_s1_wgrad(dy.data_ptr(), xn.data_ptr(), buf[8:].data_ptr(), S, N, H, W, Cp, Co, s),
                 "wgrad")
    X.assert_guard_1d(buf, 8, 8 + S * Co * Cp, f"{tag} wgrad slabs")
    g1, g2 = torch.empty(nw, device=gpu), torch.empty(nw, device=gpu)
    K.conv1x1_s1_wgrad(dy, xn, Co, Ci, out=g1)
    K.conv1x1_s1_wgrad(dy, xn, Co, Ci, out=g2)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), f"{tag} wgrad not reproducible"
    # SGD: buf = mom*buf0 + (g + wd*w0), p = w0 - lr*buf in float64 with the fp32 hyper-parameters; the kernel rounds
    # three fp32 fmas, each within half an ulp (2**-24 relative) of a value bounded by the terms' magnitudes
    torch.manual_seed(nw)
    w0 = (torch.randn(Co, Ci) * 0.05).to(F32)
    b0 = (torch.randn(Co, Ci) * 0.5).to(F32)
    lr = torch.tensor(0.1, dtype=F32)
    mom, wdec = torch.tensor(0.9, dtype=F32).double(), torch.tensor(5e-4, dtype=F32).double()
    p, mb = w0.to(gpu), b0.to(gpu)
    K.conv1x1_s1_wgrad(dy, xn, Co, Ci, sgd=(p, mb, None, lr.to(gpu), float(mom), float(wdec)))
    buf_ref = mom * b0.double() + (c["dw"] + wdec * w0.double())
    p_ref = w0.double() - lr.double() * buf_ref
    eps = 2.0 ** -24
    tol_b = 4 * eps * ((mom * b0.double()).abs() + c["dw"].abs() + (wdec * w0.double()).abs()) + 1e-30
    tol_p = lr.double() * tol_b + 2 * eps * (w0.double().abs() + lr.double() * buf_ref.abs())
    assert bool(((mb.double().cpu() - buf_ref).abs() <= tol_b).all()), f"{tag} fused SGD momentum"
    assert bool(((p.double().cpu() - p_ref).abs() <= tol_p).all()), f"{tag} fused SGD parameter"


def test_conv1x1_s1_refusals(gpu):
    """Outside the supported range: a negative code from the C entry points, an exception from the wrappers."""
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    lib = native.kernels()
    s = native.stream_handle()
    z = torch.zeros(256 * 256, dtype=BF16, device=gpu)
    p = z.data_ptr()
    assert lib.ddpx_conv1x1_s1_fwd(p, p, p, 1, 2, 2, 256, 256, s) < 0      # the weight is 128 KiB
    assert lib.ddpx_conv1x1_s1_dgrad(p, p, p, 1, 2, 2, 256, 256, s) < 0
    assert lib.ddpx_conv1x1_s1_wgrad_slabs(1, 2, 2, 256, 256) < 0
    assert lib.ddpx_conv1x1_s1_wgrad_slabs(1, 2, 2, 8, 1024) < 0           # the staging chunk is over 64 KiB
    assert lib.ddpx_conv1x1_s1_fwd(p, p, p, 1, 2, 2, 12, 8, s) < 0
    assert lib.ddpx_conv1x1_s1_fwd(p, p, p, 1, 0, 2, 8, 8, s) < 0
    assert lib.ddpx_conv1x1_s1_fwd(p + 2, p, p, 1, 2, 2, 8, 8, s) < 0
    x = z[:4 * 256].view(1, 2, 2, 256)
    with pytest.raises(native.NativeError):
        K.conv1x1_s1_fwd(x, z, 256)
    with pytest.raises(native.NativeError):
        K.conv1x1_s1_dgrad(x.view(4, 256), z, 1, 2, 2, 256, 256)
    with pytest.raises(native.NativeError):
        K.conv1x1_s1_wgrad(x.view(4, 256), x, 256, 256, out=torch.empty(256 * 256, device=gpu))
    with pytest.raises(ValueError):
        K.conv1x1_s1_fwd(z[:32].view(1, 2, 2, 8), z[:64], 8, stats=True)
