"""Element-exact tests of the implicit-GEMM 3x3 convolutions (csrc/kernels/conv_igemm*.hip on ddpx_pipe.h):
forward (+ per-tile BatchNorm statistics, + bias/ReLU), data gradient (+ ReLU mask and column sums) and weight
gradient, on non-square geometries, with integer operands (tests/_exact.py) against float64 references."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CONV_CFGS = tuple(range(16)) + (21, 22, 23, 24, 25)  # 16 - 20 are the plain-operand warp-specialised rings


def _id(v):
    return "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def _dev_case(geom, chans):
    """Device operands of a case (read-only): NHWC x padded to Cp channels, prepared weights, dy, bias."""
    from ddpx.ops import conv as K
    dev = torch.device("cuda", 0)
    c = X.conv_case(geom, chans)
    Ci, Co = chans
    Cp = X.padded_channels(Ci)
    assert Cp == K.padded_channels(Ci)
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, 9 * Cp, "conv fwd")
    X.require_exact(X.CONV_XMAX, X.CONV_WMAX, 9 * Co, "conv dgrad")
    X.require_exact(X.CONV_XMAX, X.CONV_XMAX, geom[0] * geom[1] * geom[2], "conv wgrad")
    xn = F.pad(c["x"], (0, Cp - Ci)).to(BF16).to(dev).contiguous()
    wf = torch.empty(Co * 9 * Cp, dtype=BF16, device=dev)
    wd = torch.empty_like(wf)
    K.weight_prep(c["w"].to(F32).to(dev), wf, wd)
    P = xn.shape[0] * xn.shape[1] * xn.shape[2]
    return dict(xn=xn, wf=wf, wd=wd, dy=c["dy"].reshape(P, Co).to(BF16).to(dev), bias=c["bias"].to(F32).to(dev),
                Cp=Cp, P=P, dx_pad=F.pad(c["dx"], (0, Cp - Ci)))


def _check_forward(K, geom, chans, tile, tag):
    N, H, W = geom
    Ci, Co = chans
    c, d = X.conv_case(geom, chans), _dev_case(geom, chans)
    P = d["P"]
    want = X.rounded(c["y"].reshape(P, Co), BF16)
    y0, _, _, _ = K.conv_fwd(d["xn"], d["wf"], Co, stats=False, tile=tile)
    X.assert_equal(y0, want, f"{tag} conv_fwd")
    y, st, T, BM = K.conv_fwd(d["xn"], d["wf"], Co, stats=True, tile=tile)
    X.assert_equal(y, want, f"{tag} conv_fwd with statistics")
    # EVERY tile's (mean, M2) row against a float64 reduction of the stored y over that tile's rows
    assert T == (P + BM - 1) // BM and tuple(st.shape) == (T, 2, Co)
    yd, sd = y.double().cpu(), st.double().cpu()
    for t in range(T):
        rows = yd[t * BM:min((t + 1) * BM, P)]
        if rows.shape[0] == 0:  # a tile row wholly past P reads zero
            assert torch.all(sd[t] == 0), f"{tag} statistics row {t} past P"
            continue
        mean = rows.mean(0)
        m2 = ((rows - mean) ** 2).sum(0)
        assert torch.allclose(sd[t, 0], mean, rtol=1e-3, atol=1e-3), \
            f"{tag} tile {t}/{T} mean: max err {float((sd[t, 0] - mean).abs().max())}"
        assert torch.allclose(sd[t, 1], m2, rtol=2e-3, atol=1e-2), \
            f"{tag} tile {t}/{T} M2: max err {float((sd[t, 1] - m2).abs().max())}"
    act = K.conv_fwd_act(d["xn"], d["wf"], Co, d["bias"], tile=tile)
    X.assert_equal(act, X.rounded((c["y"] + c["bias"]).clamp_min(0).reshape(P, Co), BF16), f"{tag} conv_fwd_act")


def _check_dgrad(K, geom, chans, tile, tag):
    from ddpx.runtime import native
    N, H, W = geom
    Ci, Co = chans
    d = _dev_case(geom, chans)
    P, Cp = d["P"], d["Cp"]
    want = X.rounded(d["dx_pad"], BF16)  # padded input channels: exactly zero
    dx = K.conv_dgrad(d["dy"], d["wd"], N, H, W, Cp, Co, tile=tile)
    X.assert_equal(dx, want, f"{tag} conv_dgrad")
    lib = native.kernels()
    lib.ddpx_conv_set_rowcache(0)  # per-chunk im2col addressing instead of the cached rows: same bytes
    try:
        dx2 = K.conv_dgrad(d["dy"], d["wd"], N, H, W, Cp, Co, tile=tile)
        y2, _, _, _ = K.conv_fwd(d["xn"], d["wf"], Co, stats=False, tile=tile)
    finally:
        lib.ddpx_conv_set_rowcache(-1)
    X.assert_equal(dx2, want, f"{tag} conv_dgrad, row cache off")
    X.assert_equal(y2, X.rounded(X.conv_case(geom, chans)["y"].reshape(P, Co), BF16), f"{tag} conv_fwd, row cache off")
    # ReLU mask of the block below in the epilogue, with its bias gradient as column sums
    mask, pos = X.mask_operand((P, Cp), P * 3 + Cp)
    dz_want = want.double().reshape(P, Cp) * pos
    dz, (part, T) = K.conv_dgrad_act(d["dy"], d["wd"], N, H, W, Cp, Co, mask.to(dx.device), tile=tile)
    X.assert_equal(dz, dz_want.to(F32).to(BF16), f"{tag} conv_dgrad_act")
    sums = dz_want.sum(0)
    assert dz_want.abs().sum(0).max() < X.EXACT_LIMIT  # integer column sums: exact in any order
    for dt in (F32, BF16):
        o = torch.full((Cp,), 555.0, dtype=dt, device=dx.device)
        K.colsum_finish(part, T, Cp, out=o)
        X.assert_equal(o, X.rounded(sums, dt), f"{tag} colsum_finish {dt} stored")
        K.colsum_finish(part, T, Cp, out=o, accumulate=True)
        X.assert_equal(o, X.rounded(sums, dt) * 2, f"{tag} colsum_finish {dt} accumulated")


def _check_wgrad(K, geom, chans, tile, tag):
    Ci, Co = chans
    c, d = X.conv_case(geom, chans), _dev_case(geom, chans)
    n = Co * Ci * 9
    dev = d["dy"].device
    c0 = X.ints((Co, Ci, 3, 3), -8, 8, n)
    for dt in (F32, BF16):
        for acc in (False, True):
            buf = torch.full((n + 16,), X.SENTINEL[dt], dtype=dt, device=dev)
            out = buf[8:8 + n]
            if acc:
                out.copy_(c0.reshape(-1).to(dt))
            K.conv_wgrad(d["dy"], d["xn"], Co, Ci, out=out, accumulate=acc, tile=tile)
            what = f"{tag} conv_wgrad {dt} accumulate {acc}"
            X.assert_equal(out.view(Co, Ci, 3, 3), X.rounded(c["dw"] + (c0 if acc else 0), dt), what)
            X.assert_guard_1d(buf, 8, 8 + n, what)


@pytest.mark.parametrize("geom,chans", X.conv_pairs(), ids=lambda v: _id(v))
def test_conv_exact_default_tile(gpu, geom, chans):
    from ddpx.ops import conv as K
    tag = f"conv {_id(geom)} {chans[0]}->{chans[1]}"
    _check_forward(K, geom, chans, -1, tag)
    _check_dgrad(K, geom, chans, -1, tag)
    _check_wgrad(K, geom, chans, -1, tag)


@pytest.mark.parametrize("cfg", CONV_CFGS)
@pytest.mark.parametrize("chans", X.CONV_CHANNELS, ids=lambda v: _id(v))
def test_conv_exact_every_config(gpu, chans, cfg):
    from ddpx.ops import conv as K
    for geom in X.CONV_CFG_GEOMS:
        tag = f"conv {_id(geom)} {chans[0]}->{chans[1]} cfg {cfg}"
        _check_forward(K, geom, chans, cfg, tag)
        _check_dgrad(K, geom, chans, cfg, tag)
        _check_wgrad(K, geom, chans, cfg, tag)


@pytest.mark.parametrize("geom", X.CONV_CFG_GEOMS, ids=lambda v: _id(v))
@pytest.mark.parametrize("chans", X.WGRAD_CHANNELS, ids=lambda v: _id(v))
def test_conv_wgrad_shared_output_reduce(gpu, chans, geom):
    """Input-channel counts whose last 64-channel tile of the reduce holds 4 / 8 channels: 4 / 2 threads share an
    output (68 real channels in 72 padded; 72)."""
    from ddpx.ops import conv as K
    for tile in (-1, 7, 12, 13, 22):
        _check_wgrad(K, geom, chans, tile, f"wgrad {_id(geom)} {chans[0]}->{chans[1]} tile {tile}")


def test_conv_rejects_warp_specialised_configs(gpu):
    """Configs 16 - 20 have no im2col variant: the entry points refuse them instead of computing something."""
    from ddpx.ops import conv as K
    from ddpx.runtime import native
    geom, chans = (2, 5, 3), (8, 8)
    d = _dev_case(geom, chans)
    for cfg in (16, 17, 18, 19, 20):
        with pytest.raises(native.NativeError):
            K.conv_fwd(d["xn"], d["wf"], 8, stats=False, tile=cfg)
        with pytest.raises(native.NativeError):
            K.conv_dgrad(d["dy"], d["wd"], *geom, 8, 8, tile=cfg)
