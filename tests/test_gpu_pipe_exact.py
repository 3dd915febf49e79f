"""Element-exact tests of the pipelined bf16 MFMA GEMM (csrc/include/ddpx_pipe.h) on plain operands.

Integer operands (tests/_exact.py): every tile config, every operand layout and every epilogue must equal the
float64 reference element for element; NaN-poisoned operand padding turns an overread into a NaN in the
output, and a sentinel-filled guard band around the output catches any store outside [0:M, 0:N]."""
import functools

import pytest
import torch

from tests import _exact as X

pytestmark = pytest.mark.gpu

LAYOUTS = {"kk": (True, True), "kn": (True, False), "mk": (False, True), "mn": (False, False)}
F32, BF16 = torch.float32, torch.bfloat16
SPLIT_TILES = (0, 5, 6, 8, 10, 14, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Logical A [M,K], B [N,K], the exact product, integers to accumulate onto, a bias: computed once per shape."""
    X.require_exact(X.GEMM_AMAX, X.GEMM_BMAX, K, f"gemm {M}x{N}x{K}")
    s = (M * 131 + N) * 131 + K
    A = X.ints((M, K), -X.GEMM_AMAX, X.GEMM_AMAX, s)
    B = X.ints((N, K), -X.GEMM_BMAX, X.GEMM_BMAX, s + 1)
    return dict(A=A, B=B, ref=A @ B.t(), c0=X.ints((M, N), -8, 8, s + 2), bias=X.ints((N,), -8, 8, s + 3))


def _shapes(cfg, ak, bk):
    from ddpx.ops import gemm as G
    bm, bn = G.tile_dims(cfg)
    shapes = [(8, 8), (bm + 8, bn + 8)]
    if ak or bk:  # a ragged last quad of rows / columns where the layout allows an extent that is no multiple of 8
        shapes.append((bm + 5 if ak else bm + 8, bn + 3 if bk else bn + 8))
    return bn, shapes


def _operands(c, ak, bk, dev):
    a = X.poisoned(c["A"] if ak else c["A"].t(), dev)
    b = X.poisoned(c["B"] if bk else c["B"].t(), dev)
    return a, b


def _raw(G, a, b, out, M, N, K, ak, bk, epi, ldc, **kw):
    return G.gemm_raw(a, b, out, M=M, N=N, K=K, lda=a.stride(0), ldb=b.stride(0), ldc=ldc, a_kcontig=ak,
                      b_kcontig=bk, epi=epi, **kw)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cfg", range(26))
def test_gemm_exact(gpu, cfg, layout):
    from ddpx.ops import gemm as G
    ak, bk = LAYOUTS[layout]
    bn, shapes = _shapes(cfg, ak, bk)
    for (M, N) in shapes:
        for K in X.GEMM_KS:
            c = _case(M, N, K)
            a, b = _operands(c, ak, bk, gpu)
            tag = f"cfg {cfg} {layout} M={M} N={N} K={K}"
            for epi, dt in ((G.EPI_F32, F32), (G.EPI_BF16, BF16)):
                for acc in (False, True):
                    # ldc = N + 5 (fp32, stored): an odd leading dimension takes the all-scalar epilogue when N is a
                    # multiple of 4, and the vector epilogue with a ragged last quad when N = bn + 3
                    for ldc in ((N + 8, N + 5) if (dt == F32 and not acc) else (N + 8,)):
                        buf, out = X.guarded(M, N, dt, gpu, ldc)
                        if acc:
                            out.copy_(c["c0"].to(dt))
                        _raw(G, a, b, out, M, N, K, ak, bk, epi, ldc, accumulate=acc, tile=cfg)
                        want = X.rounded(c["ref"] + (c["c0"] if acc else 0), dt)
                        what = f"{tag} epi {epi} acc {acc} ldc {ldc}"
                        X.assert_equal(out, want, what)
                        X.assert_guard(buf, M, N, what)
            if layout == "kk":
                _forward_epilogues(G, c, a, b, M, N, cfg, bn, gpu, tag)
            if layout == "kn":
                _dgrad_epilogues(G, c, a, b, M, N, K, cfg, gpu, tag)


def _forward_epilogues(G, c, x, w, M, N, cfg, bn, dev, tag):
    """bias / bias + ReLU -> bf16, bias -> fp32 through ``linear_fwd`` into a column slice of a wider activation
    (what ddpx/ops/mlp.py does with ``out=h[:, r0:r1]``): the slice is exact, its neighbours are untouched."""
    bias = c["bias"].to(F32).to(dev)
    z = c["ref"] + c["bias"]
    for c0 in (8, bn + 8):
        wide_ld = (c0 + N + 8 + 7) // 8 * 8
        for relu, dt in ((False, BF16), (True, BF16), (False, F32)):
            buf, out = X.guarded(M, N, dt, dev, wide_ld, c0=c0)
            G.linear_fwd(x, w, bias=bias, relu=relu, out=out, out_dtype=dt, tile=cfg)
            what = f"{tag} linear_fwd relu {relu} {dt} slice at column {c0} of {wide_ld}"
            X.assert_equal(out, X.rounded(z.clamp_min(0) if relu else z, dt), what)
            X.assert_guard(buf, M, N, what, c0=c0)
    buf, out = X.guarded(M, N, BF16, dev, (8 + N + 8 + 7) // 8 * 8, c0=8)  # no bias: EPI_BF16 into a slice
    G.linear_fwd(x, w, out=out, tile=cfg)
    X.assert_equal(out, X.rounded(c["ref"], BF16), f"{tag} linear_fwd plain slice")
    X.assert_guard(buf, M, N, f"{tag} linear_fwd plain slice", c0=8)


def _dgrad_epilogues(G, c, dy, w, M, N, K, cfg, dev, tag):
    """``linear_dgrad``: the ReLU-mask epilogue (mask operand with positive, negative, +0 and -0 values) and the
    bias gradient of the layer below: the column sums of the stored dX, finished in the launch on the 4-wave and
    warp-specialised tiles and from the partial rows on the 8-wave ones.  Sums of integers: no tolerance."""
    if N % 8:
        return  # B is N-contiguous here: N is a multiple of 8 in every shape of this layout
    mask, pos = X.mask_operand((M, N), M * 7 + N)
    mk = X.poisoned(mask, dev)
    mk[:] = mask.to(dev)  # (exact bits: -0 survives)
    dx_want = X.rounded(c["ref"], BF16).double() * pos
    sums = dx_want.sum(0)  # what the kernel stored is integer-valued: its column sums are exact in fp32
    assert sums.abs().max() < X.EXACT_LIMIT
    for dt in (F32, BF16):
        buf = torch.full((M + 2, N), X.SENTINEL[BF16], dtype=BF16, device=dev)
        out = buf[1:M + 1]
        bg = torch.full((N,), 777.0, dtype=dt, device=dev)
        # linear_dgrad(dy [M, K'], w [K', N]): the GEMM's K is dy's inner extent
        G.linear_dgrad(dy, w, relu_mask_of=mk, out=out, tile=cfg, bias_grad=bg)
        what = f"{tag} linear_dgrad mask bias_grad {dt}"
        X.assert_equal(out, dx_want.to(F32).to(BF16), what)
        X.assert_guard(buf, M, N, what)
        X.assert_equal(bg, X.rounded(sums, dt), what + " stored")
        G.linear_dgrad(dy, w, relu_mask_of=mk, out=out, tile=cfg, bias_grad=bg, bias_grad_accumulate=True)
        X.assert_equal(bg, X.rounded(sums, dt) * 2, what + " accumulated: twice the stored")
    out = G.linear_dgrad(dy, w, tile=cfg)  # no mask: EPI_BF16
    X.assert_equal(out, X.rounded(c["ref"], BF16), f"{tag} linear_dgrad plain")


@pytest.mark.parametrize("layout", ["kk", "kn"])
@pytest.mark.parametrize("cfg", SPLIT_TILES)
def test_gemm_forced_splitk_exact(gpu, cfg, layout):
    """In-launch split-K with uneven slices (K = 904: 512+392, 320+320+264, 256*3+136), three runs each: the
    result is the reference every time (the last split of a tile resets its ticket)."""
    from ddpx.ops import gemm as G
    ak, bk = LAYOUTS[layout]
    _, shapes = _shapes(cfg, ak, bk)
    K = 904
    for (M, N) in shapes[1:]:
        c = _case(M, N, K)
        a, b = _operands(c, ak, bk, gpu)
        for splits in (2, 3, 4):
            for epi, dt in ((G.EPI_F32, F32), (G.EPI_BF16, BF16)):
                want = X.rounded(c["ref"], dt)
                for run in range(3):
                    buf, out = X.guarded(M, N, dt, gpu)
                    _raw(G, a, b, out, M, N, K, ak, bk, epi, N + 8, tile=cfg, splits=splits)
                    what = f"cfg {cfg} {layout} M={M} N={N} splits {splits} epi {epi} run {run}"
                    X.assert_equal(out, want, what)
                    X.assert_guard(buf, M, N, what)
        if layout == "kk":  # the forward's bias + ReLU epilogue behind the combine
            bias = c["bias"].to(F32).to(gpu)
            buf, out = X.guarded(M, N, BF16, gpu, (N + 16 + 7) // 8 * 8, c0=8)
            G.linear_fwd(a, b, bias=bias, relu=True, out=out, tile=cfg, splits=3)
            X.assert_equal(out, X.rounded((c["ref"] + c["bias"]).clamp_min(0), BF16), f"cfg {cfg} split fwd")
            X.assert_guard(buf, M, N, f"cfg {cfg} split fwd", c0=8)
