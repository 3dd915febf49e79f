"""Element-exact tests of the fp32 stride-2 convolutions (csrc/kernels/f32_conv_s2.hip): 3x3 / pad 1 and 1x1 / pad 0,
forward (+ per-tile BatchNorm statistics), parity-class data gradient and split-K weight gradient, with integer
operands (tests/_exact.py) against float64 ``F.conv2d(stride=2)`` and its CPU autograd; one real-valued case per
kernel size at the stride-1 fp32 convolutions' error bar."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

pytestmark = pytest.mark.gpu

NAN = float("nan")
BIG = (9, 8, 8)  # more than one forward row tile, row tile per parity class and weight-gradient split on both tiles
# (kernel size, (N, H, W), (Ci, Co), tile).  tile 0 / 1 force the 128x128 / 64x64 tile; the default (-1) takes 64x64
# at all of these sizes.
CASES = (
    (3, (2, 1, 1), (4, 4), -1), (3, (1, 2, 2), (8, 12), -1), (3, (3, 1, 8), (20, 36), -1),
    (3, (1, 3, 5), (16, 16), -1), (3, (2, 5, 3), (64, 68), -1), (3, (3, 7, 7), (32, 132), -1),
    (3, (2, 12, 12), (20, 36), -1), (3, (2, 12, 12), (3, 16), -1), (3, BIG, (64, 68), 0), (3, BIG, (32, 132), 1),
    (3, BIG, (20, 36), 0), (3, (2, 5, 3), (20, 36), 0), (3, (3, 7, 7), (64, 68), 0), (3, (3, 7, 7), (8, 12), 1),
    (3, (2, 12, 12), (32, 132), 1),
    (1, (2, 1, 1), (8, 12), -1), (1, (1, 2, 2), (4, 4), -1), (1, (3, 1, 8), (16, 16), -1),
    (1, (1, 3, 5), (20, 36), -1), (1, (2, 5, 3), (32, 132), -1), (1, (3, 7, 7), (64, 68), -1),
    (1, (2, 12, 12), (64, 68), 0), (1, BIG, (32, 132), 1), (1, BIG, (20, 36), 0), (1, (2, 5, 3), (8, 12), 0),
)
IDS = ["%dx%d-%s-%s-t%d" % (k, k, "x".join(map(str, g)), "to".join(map(str, c)), t) for k, g, c, t in CASES]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _case(ks, geom, chans, real=False):
    """Operands (float64, CPU) and float64 references of one case, computed once (read-only): x [N,H,W,Ci],
    w [Co,Ci,k,k], dy [N,Ho,Wo,Co]; y, dx (NHWC), dw."""
    (N, H, W), (Ci, Co) = geom, chans
    s = ((((ks * 16 + N) * 32 + H) * 32 + W) * 256 + Ci) * 256 + Co  # one seed per case, from its numbers
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if real:
        g = torch.Generator().manual_seed(s)
        x = torch.randn(N, H, W, Ci, generator=g).double()
        w = (torch.randn(Co, Ci, ks, ks, generator=g) * (Ci * ks * ks) ** -0.5).double()
        dy = torch.randn(N, Ho, Wo, Co, generator=g).double()
    else:
        x = X.ints((N, H, W, Ci), -X.CONV_XMAX, X.CONV_XMAX, s)
        w = X.ints((Co, Ci, ks, ks), -X.CONV_WMAX, X.CONV_WMAX, s + 1)
        dy = X.ints((N, Ho, Wo, Co), -X.CONV_XMAX, X.CONV_XMAX, s + 2)
    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = F.conv2d(xc, wr, stride=2, padding=ks // 2)
    assert tuple(y.shape[2:]) == (Ho, Wo)
    dx, dw = torch.autograd.grad(y, (xc, wr), dy.permute(0, 3, 1, 2))
    return dict(x=x, w=w, dy=dy, y=y.detach().permute(0, 2, 3, 1).reshape(-1, Co), dx=dx.permute(0, 2, 3, 1), dw=dw)


def _inside(t, gpu):
    """t as a contiguous 16-B aligned fp32 view inside a larger NaN-filled allocation: an over-read shows as NaN."""
    buf = torch.full((t.numel() + 32,), NAN, dtype=torch.float32, device=gpu)
    v = buf[16:16 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run(gpu, ks, geom, chans, tile, c, check):
    """All three kernels of one case; ``check(got, want, what)`` compares each result with its reference."""
    from ddpx.ops import f32 as K
    from ddpx.runtime import native
    lib = native.kernels()
    (N, H, W), (Ci, Co) = geom, chans
    Cp, Ho, Wo, T2 = K.conv_channels(Ci), (H + 1) // 2, (W + 1) // 2, ks * ks
    P = N * Ho * Wo
    tag = f"{ks}x{ks}/s2 {geom} {Ci}->{Co} tile {tile}"
    xn = _inside(F.pad(c["x"], (0, Cp - Ci)), gpu)
    dy = _inside(c["dy"].reshape(P, Co), gpu)
    w = _inside(c["w"], gpu)
    wf = _inside(torch.zeros(T2 * Cp * Co), gpu)
    wd = _inside(torch.zeros(T2 * Co * Ci), gpu) if Ci == Cp else None
    if ks == 3:
        K.conv_wprep(w, wf, wd)
        fwd = lambda st: K.conv_s2_fwd(xn, wf, Co, stats=st, tile=tile)
        wgrad = lambda out, acc: K.conv_s2_wgrad(dy, xn, Co, Ci, out, accumulate=acc, tile=tile)
    else:
        K.conv1x1_wprep(w, wf)
        wd = w  # the data gradient reads the master itself
        fwd = lambda st: K.conv1x1_s2_fwd(xn, wf, Co, stats=st, tile=tile)
        wgrad = lambda out, acc: K.conv1x1_s2_wgrad(dy, xn, Co, Ci, out, accumulate=acc, tile=tile)
    if geom == BIG:
        for t in (0, 1):
            bm = lib.ddpx_f32_conv_s2_fwd_tile_rows(N, H, W, Cp, Co, ks, t)
            per_class = -(-N * (H // 2) * (W // 2) // bm)
            assert lib.ddpx_f32_conv_s2_fwd_tiles_m(N, H, W, Cp, Co, ks, t) > 1
            assert per_class > 1 and lib.ddpx_f32_conv_s2_dgrad_tiles_m(N, H, W, Cp, Co, ks, t) == 4 * per_class
            assert lib.ddpx_f32_conv_s2_wgrad_splits(N, H, W, Cp, Co, ks, t) > 1

    # ---- forward without and with statistics; every tile's (mean, M2) against float64 over its stored rows
    y0, none = fwd(False)
    assert none is None
    check(y0, c["y"], f"{tag} forward")
    y, (st, T, R) = fwd(True)
    check(y, c["y"], f"{tag} forward with statistics")
    assert T == (P + R - 1) // R and tuple(st.shape) == (T, 2, Co)
    yd = y.double().cpu()
    for t in range(T):
        rows = yd[t * R:min((t + 1) * R, P)]
        mean = rows.mean(0)
        m1, m2 = _rel(st[t, 0], mean), _rel(st[t, 1], ((rows - mean) ** 2).sum(0))
        assert m1 < 1e-5 and m2 < 1e-5, f"{tag} tile {t}/{T}: mean {m1:.2e}, M2 {m2:.2e}"

    # ---- data gradient over the whole [N, H, W, C] (the 1x1's three zero quarters included): the wrapper, then the
    # C entry point on NaN-filled storage with NaN behind it: an unwritten or overrun element shows
    if Ci == Cp:
        dgrad = K.conv_s2_dgrad if ks == 3 else K.conv1x1_s2_dgrad
        check(dgrad(dy, wd, N, H, W, Cp, Co, tile=tile), c["dx"], f"{tag} dgrad")
        n = N * H * W * Cp
        buf = torch.full((n + 64,), NAN, dtype=torch.float32, device=gpu)
        native.check(lib.ddpx_f32_conv_s2_dgrad(dy.data_ptr(), wd.data_ptr(), buf.data_ptr(), N, H, W, Cp, Co, ks, tile,
                                                native.stream_handle()), "ddpx_f32_conv_s2_dgrad")
        check(buf[:n].view(N, H, W, Cp), c["dx"], f"{tag} dgrad on NaN-filled storage")
        assert bool(torch.isnan(buf[n:]).all()), f"{tag} dgrad wrote past dx"

    # ---- weight gradient in torch layout: stored / accumulated inside sentinels, bitwise reproducible
    nw = Co * Ci * T2
    c0 = X.ints((Co, Ci, ks, ks), -8, 8, nw)
    outs = []
    for acc in (False, True, False):
        buf = torch.full((nw + 16,), X.SENTINEL[torch.float32], dtype=torch.float32, device=gpu)
        out = buf[8:8 + nw]
        if acc:
            out.copy_(c0.reshape(-1))
        wgrad(out, acc)
        check(out.view(Co, Ci, ks, ks), c["dw"] + (c0 if acc else 0), f"{tag} wgrad accumulate {acc}")
        X.assert_guard_1d(buf, 8, 8 + nw, f"{tag} wgrad accumulate {acc}")
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)), f"{tag} wgrad not reproducible"


@pytest.mark.parametrize("ks,geom,chans,tile", CASES, ids=IDS)
def test_f32_conv_s2_exact(gpu, ks, geom, chans, tile):
    (N, H, W), (Ci, Co) = geom, chans
    # integer operands: every fp32 product and partial sum stays an integer below 2**24 in any order
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, ks * ks * Ci, "fwd")
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, (4 if ks == 3 else 1) * Co, "dgrad")
    X.require_exact(X.CONV_XMAX, X.CONV_XMAX, N * ((H + 1) // 2) * ((W + 1) // 2), "wgrad")
    _run(gpu, ks, geom, chans, tile, _case(ks, geom, chans),
         lambda got, want, what: X.assert_equal(got, want.to(torch.float32), what))


@pytest.mark.parametrize("ks", (3, 1))
def test_f32_conv_s2_real(gpu, ks):
    """Real-valued operands at the bar of tests/test_gpu_f32.py::test_conv_fwd_dgrad_wgrad (same instruction, same
    summation order): a wrong block order that still sums every term passes the integer cases, not this one."""
    def check(got, want, what):
        assert got.shape == want.shape and _rel(got, want) < 1e-5, f"{what}: relative L2 error {_rel(got, want):.3e}"
    _run(gpu, ks, (8, 16, 16), (64, 128), -1, _case(ks, (8, 16, 16), (64, 128), real=True), check)


def test_f32_conv_s2_refusals(gpu):
    """Unsupported shapes and unknown tiles: a negative code from every C entry point, an exception from the
    wrappers."""
    from ddpx.ops import f32 as K
    from ddpx.runtime import native
    lib = native.kernels()
    x = torch.zeros(1, 4, 4, 8, device=gpu)
    wf = torch.zeros(9 * 8 * 8, device=gpu)
    dy = torch.zeros(4, 8, device=gpu)
    s = native.stream_handle()
    a, b, c = x.data_ptr(), wf.data_ptr(), dy.data_ptr()
    for bad in ((1, 4, 4, 6, 8, 3, -1), (1, 4, 4, 8, 6, 3, -1), (1, 0, 4, 8, 8, 3, -1), (1, 4, 4, 8, 8, 2, -1),
                (1, 4, 4, 8, 8, 3, 2), (1, 4, 4, 8, 8, 3, -2), (1, 4, 4, 8, 8, 1, 7), (1, 4, 4, 6, 8, 1, -1)):
        assert lib.ddpx_f32_conv_s2_fwd_tile_rows(*bad) < 0, bad
        assert lib.ddpx_f32_conv_s2_fwd_tiles_m(*bad) < 0, bad
        assert lib.ddpx_f32_conv_s2_dgrad_tiles_m(*bad) < 0, bad
        assert lib.ddpx_f32_conv_s2_wgrad_splits(*bad) < 0, bad
        assert lib.ddpx_f32_conv_s2_fwd(a, b, c, None, *bad, s) < 0, bad
        assert lib.ddpx_f32_conv_s2_dgrad(c, b, a, *bad, s) < 0, bad
        assert lib.ddpx_f32_conv_s2_wgrad(c, a, b, 1, *bad, s) < 0, bad
    x6 = torch.zeros(1, 4, 4, 6, device=gpu)
    with pytest.raises(ValueError):
        K.conv_s2_fwd(x6, wf[:9 * 6 * 8], 8, stats=False)
    with pytest.raises(ValueError):
        K.conv1x1_s2_dgrad(dy, torch.zeros(8, 6, 1, 1, device=gpu), 1, 4, 4, 6, 8)
    for tile in (2, -2):
        with pytest.raises(native.NativeError):
            K.conv_s2_fwd(x, wf, 8, stats=True, tile=tile)
        with pytest.raises(native.NativeError):
            K.conv_s2_dgrad(dy, wf, 1, 4, 4, 8, 8, tile=tile)
        with pytest.raises(native.NativeError):
            K.conv_s2_wgrad(dy, x, 8, 8, torch.empty(8 * 8 * 9, device=gpu), tile=tile)
