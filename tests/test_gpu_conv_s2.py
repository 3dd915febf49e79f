"""Element-exact tests of the stride-2 convolutions (csrc/kernels/conv_igemm_s2.hip): 3x3 / pad 1 and 1x1 / pad 0,
forward (+ per-tile BatchNorm statistics), parity-class data gradient and split-K weight gradient, with integer
operands (tests/_exact.py) against float64 ``F.conv2d(stride=2)`` and its CPU autograd."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16

# (kernel size, (N, H, W), (Ci, Co), tile): every geometry and every channel pair for both kernels; tile 0 / 1 name
# the 128x128 / 64x64 tile where the default would not pick it
CASES = (
    (3, (2, 1, 1), (8, 8), -1), (3, (1, 2, 2), (16, 24), -1), (3, (3, 1, 8), (64, 64), -1),
    (3, (1, 3, 5), (24, 40), -1), (3, (2, 5, 3), (64, 136), -1), (3, (3, 7, 7), (128, 72), -1),
    (3, (2, 12, 12), (16, 24), -1), (3, (5, 16, 16), (64, 136), -1), (3, (5, 16, 16), (8, 8), -1),
    (3, (2, 5, 3), (24, 40), 0), (3, (3, 7, 7), (128, 72), 0), (3, (5, 16, 16), (64, 136), 0),
    (3, (5, 16, 16), (128, 72), 1),
    (1, (2, 1, 1), (16, 24), -1), (1, (1, 2, 2), (8, 8), -1), (1, (3, 1, 8), (24, 40), -1),
    (1, (1, 3, 5), (64, 64), -1), (1, (2, 5, 3), (128, 72), -1), (1, (3, 7, 7), (64, 136), -1),
    (1, (2, 12, 12), (64, 64), -1), (1, (5, 16, 16), (128, 72), -1), (1, (5, 16, 16), (16, 24), -1),
)


@functools.lru_cache(maxsize=None)
def _case(ks, geom, chans):
    """Operands (float64, CPU) and references of one case, computed once (read-only): x [N,H,W,Ci], w [Co,Ci,k,k],
    dy [N,Ho,Wo,Co]; y, dx (NHWC), dw."""
    N, H, W = geom
    Ci, Co = chans
    s = ((((ks * 8 + N) * 32 + H) * 32 + W) * 256 + Ci) * 256 + Co  # one seed per case, from its numbers
    x = X.ints((N, H, W, Ci), -X.CONV_XMAX, X.CONV_XMAX, s)
    w = X.ints((Co, Ci, ks, ks), -X.CONV_WMAX, X.CONV_WMAX, s + 1)
    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = F.conv2d(xc, wr, stride=2, padding=ks // 2)
    Ho, Wo = y.shape[2], y.shape[3]
    dy = X.ints((N, Ho, Wo, Co), -X.CONV_XMAX, X.CONV_XMAX, s + 2)
    dx, dw = torch.autograd.grad(y, (xc, wr), dy.permute(0, 3, 1, 2))
    return dict(x=x, w=w, dy=dy, y=y.detach().permute(0, 2, 3, 1).contiguous(), dx=dx.permute(0, 2, 3, 1).contiguous(),
                dw=dw, Ho=Ho, Wo=Wo)


def _ops(K, ks):
    """(fwd, dgrad, wgrad) of one kernel size behind one signature (the 1x1 wrappers take no tile)."""
    if ks == 3:
        return (K.conv_s2_fwd, K.conv_s2_dgrad,
                lambda dy, x, Co, Cr, tile, **kw: K.conv_s2_wgrad(dy, x, Co, Cr, tile=tile, **kw))
    return (lambda x, wf, Co, stats, tile: K.conv1x1_s2_fwd(x, wf, Co, stats=stats),
            lambda dy, wd, N, H, W, C, Co, tile: K.conv1x1_s2_dgrad(dy, wd, N, H, W, C, Co),
            lambda dy, x, Co, Cr, tile, **kw: K.conv1x1_s2_wgrad(dy, x, Co, Cr, **kw))


@pytest.mark.parametrize("ks,geom,chans,tile", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_s2_exact(gpu, ks, geom, chans, tile):
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    lib = native.kernels()
    N, H, W = geom
    Ci, Co = chans
    c = _case(ks, geom, chans)
    Ho, Wo = c["Ho"], c["Wo"]
    assert (Ho, Wo) == K.s2_out_hw(H, W)
    Cp, P = X.padded_channels(Ci), N * Ho * Wo
    T2 = ks * ks
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, T2 * Cp, "fwd")
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, (4 if ks == 3 else 1) * Co, "dgrad")
    X.require_exact(X.CONV_XMAX, X.CONV_XMAX, P, "wgrad")
    fwd, dgrad, wgrad = _ops(K, ks)
    tag = f"{ks}x{ks}/s2 {geom} {Ci}->{Co} tile {tile}"
    xn = F.pad(c["x"], (0, Cp - Ci)).to(BF16).to(gpu).contiguous()
    dy = c["dy"].reshape(P, Co).to(BF16).to(gpu)
    if ks == 3:
        wf = torch.empty(Co * 9 * Cp, dtype=BF16, device=gpu)
        wd = torch.empty_like(wf)
        K.weight_prep(c["w"].to(F32).to(gpu), wf, wd)
    else:
        wf = wd = torch.empty(Co * Cp, dtype=BF16, device=gpu)
        K.weight_prep_1x1(c["w"].to(F32).to(gpu), wf, wd)
    if geom == (5, 16, 16):  # the multi-tile / multi-split case
        assert lib.ddpx_conv_s2_fwd_tiles_m(N, H, W, Cp, Co, ks, tile) > 1
        assert lib.ddpx_conv_s2_dgrad_tiles_m(N, H, W, Cp, Co, ks, tile) > 4
        assert lib.ddpx_conv_s2_wgrad_splits(N, H, W, Cp, Co, ks, tile) > 1

    # ---- forward, and every tile's (mean, M2) against a float64 reduction of the stored y over its rows
    want = X.rounded(c["y"].reshape(P, Co), BF16)
    y0, _, _, _ = fwd(xn, wf, Co, False, tile)
    X.assert_equal(y0, want, f"{tag} forward")
    y, st, T, BM = fwd(xn, wf, Co, True, tile)
    X.assert_equal(y, want, f"{tag} forward with statistics")
    assert T == (P + BM - 1) // BM and tuple(st.shape) == (T, 2, Co)
    yd, sd = y.double().cpu(), st.double().cpu()
    for t in range(T):
        rows = yd[t * BM:min((t + 1) * BM, P)]
        mean = rows.mean(0)
        m2 = ((rows - mean) ** 2).sum(0)
        assert torch.allclose(sd[t, 0], mean, rtol=1e-3, atol=1e-3), f"{tag} tile {t}/{T} mean"
        assert torch.allclose(sd[t, 1], m2, rtol=2e-3, atol=1e-2), f"{tag} tile {t}/{T} M2"

    # ---- data gradient over the whole [N, H, W, Cp] (padded channels and the 1x1's three zero quarters included),
    # then the C entry point on NaN-filled storage with NaN behind it: an unwritten or overrun element shows
    want_dx = X.rounded(F.pad(c["dx"], (0, Cp - Ci)), BF16)
    X.assert_equal(dgrad(dy, wd, N, H, W, Cp, Co, tile), want_dx, f"{tag} dgrad")
    n = N * H * W * Cp
    dxp = X.poisoned(torch.full((1, n), float("nan")), gpu)
    native.check(lib.ddpx_conv_s2_dgrad(dy.data_ptr(), wd.data_ptr(), dxp.data_ptr(), N, H, W, Cp, Co, ks, tile,
                                        native.stream_handle()), "ddpx_conv_s2_dgrad")
    X.assert_equal(dxp.reshape(N, H, W, Cp), want_dx, f"{tag} dgrad on poisoned storage")
    assert bool(torch.isnan(dxp._base[0, n:]).all()), f"{tag} dgrad wrote past dx"

    # ---- weight gradient in torch layout: stored / accumulated, fp32 / bf16, bitwise reproducible, fused SGD
    nw = Co * Ci * T2
    c0 = X.ints((Co, Ci, ks, ks), -8, 8, nw)
    for dt in (F32, BF16):
        for acc in (False, True):
            buf = torch.full((nw + 16,), X.SENTINEL[dt], dtype=dt, device=gpu)
            out = buf[8:8 + nw]
            if acc:
                out.copy_(c0.reshape(-1).to(dt))
            wgrad(dy, xn, Co, Ci, tile, out=out, accumulate=acc)
            what = f"{tag} wgrad {dt} accumulate {acc}"
            X.assert_equal(out.view(Co, Ci, ks, ks), X.rounded(c["dw"] + (c0 if acc else 0), dt), what)
            X.assert_guard_1d(buf, 8, 8 + nw, what)
    g1, g2 = torch.empty(nw, device=gpu), torch.empty(nw, device=gpu)
    wgrad(dy, xn, Co, Ci, tile, out=g1)
    wgrad(dy, xn, Co, Ci, tile, out=g2)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), f"{tag} wgrad not reproducible"
    # SGD: buf = mom*buf0 + (g + wd*w0), p = w0 - lr*buf, in float64 with the fp32 hyper-parameters; the kernel
    # rounds three fp32 fmas, each within half an ulp (2**-24 relative) of a value bounded by the terms' magnitudes
    torch.manual_seed(nw)
    w0 = (torch.randn(Co, Ci, ks, ks) * 0.05).to(F32)
    b0 = (torch.randn(Co, Ci, ks, ks) * 0.5).to(F32)
    lr = torch.tensor(0.1, dtype=F32)
    mom, wdec = torch.tensor(0.9, dtype=F32).double(), torch.tensor(5e-4, dtype=F32).double()
    p, mb = w0.to(gpu), b0.to(gpu)
    wgrad(dy, xn, Co, Ci, tile, sgd=(p, mb, None, lr.to(gpu), float(mom), float(wdec)))
    buf_ref = mom * b0.double() + (c["dw"] + wdec * w0.double())
    p_ref = w0.double() - lr.double() * buf_ref
    eps = 2.0 ** -24
    tol_b = 4 * eps * ((mom * b0.double()).abs() + c["dw"].abs() + (wdec * w0.double()).abs()) + 1e-30
    tol_p = lr.double() * tol_b + 2 * eps * (w0.double().abs() + lr.double() * buf_ref.abs())
    assert bool(((mb.double().cpu() - buf_ref).abs() <= tol_b).all()), f"{tag} fused SGD momentum"
    assert bool(((p.double().cpu() - p_ref).abs() <= tol_p).all()), f"{tag} fused SGD parameter"


def test_conv_s2_refusals(gpu):
    """Unsupported shapes and unknown tiles: a negative code from the C entry points, an exception from the
    wrappers."""
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    lib = native.kernels()
    x = torch.zeros(1, 4, 4, 8, dtype=BF16, device=gpu)
    wf = torch.zeros(8 * 9 * 8, dtype=BF16, device=gpu)
    dy = torch.zeros(4, 8, dtype=BF16, device=gpu)
    s = native.stream_handle()
    for ks in (3, 1):
        assert lib.ddpx_conv_s2_fwd(x.data_ptr(), wf.data_ptr(), dy.data_ptr(), None, 1, 4, 4, 12, 8, ks, -1, s) < 0
        assert lib.ddpx_conv_s2_fwd(x.data_ptr(), wf.data_ptr(), dy.data_ptr(), None, 1, 0, 4, 8, 8, ks, -1, s) < 0
        assert lib.ddpx_conv_s2_dgrad(dy.data_ptr(), wf.data_ptr(), x.data_ptr(), 1, 4, 4, 12, 8, ks, -1, s) < 0
        assert lib.ddpx_conv_s2_wgrad_splits(1, 4, 4, 8, 12, ks, -1) < 0
        for tile in (2, 7, -2):
            assert lib.ddpx_conv_s2_fwd(x.data_ptr(), wf.data_ptr(), dy.data_ptr(), None, 1, 4, 4, 8, 8, ks, tile, s) < 0
            assert lib.ddpx_conv_s2_dgrad(dy.data_ptr(), wf.data_ptr(), x.data_ptr(), 1, 4, 4, 8, 8, ks, tile, s) < 0
            assert lib.ddpx_conv_s2_wgrad_splits(1, 4, 4, 8, 8, ks, tile) < 0
    x12 = torch.zeros(1, 4, 4, 12, dtype=BF16, device=gpu)
    with pytest.raises((ValueError, native.NativeError)):
        K.conv_s2_fwd(x12, wf, 8, stats=False)
    with pytest.raises((ValueError, native.NativeError)):
        K.conv1x1_s2_fwd(x12, wf[:96], 8, stats=False)
    for tile in (2, -2):
        with pytest.raises(native.NativeError):
            K.conv_s2_fwd(x, wf, 8, stats=True, tile=tile)
        with pytest.raises(native.NativeError):
            K.conv_s2_dgrad(dy, wf, 1, 4, 4, 8, 8, tile=tile)
        with pytest.raises(native.NativeError):
            K.conv_s2_wgrad(dy, x, 8, 8, out=torch.empty(8 * 8 * 9, device=gpu), tile=tile)
