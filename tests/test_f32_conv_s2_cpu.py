"""The fp32 stride-2 convolutions (ddpx.ops.f32, csrc/kernels/f32_conv_s2.hip) where no GPU is needed: the wrappers'
argument checks, and the parity-class decomposition of the data gradient on the float64 reference."""
import pytest
import torch
import torch.nn.functional as F

from tests import _exact as X


def test_wrappers_refuse_before_the_library():
    from ddpx.ops import f32 as K
    x = torch.zeros(1, 4, 4, 8)
    wf, dy, out = torch.zeros(9 * 8 * 8), torch.zeros(4, 8), torch.zeros(8 * 8 * 9)
    w1 = torch.zeros(8, 8, 1, 1)
    calls = (
        lambda: K.conv_s2_fwd(x, wf, 8),                                  # CPU tensors
        lambda: K.conv_s2_dgrad(dy, wf, 1, 4, 4, 8, 8),
        lambda: K.conv_s2_wgrad(dy, x, 8, 8, out),
        lambda: K.conv1x1_wprep(w1, wf[:64]),
        lambda: K.conv1x1_s2_fwd(x, wf[:64], 8),
        lambda: K.conv1x1_s2_dgrad(dy, w1, 1, 4, 4, 8, 8),
        lambda: K.conv1x1_s2_wgrad(dy, x, 8, 8, out[:64]),
        lambda: K.conv_s2_fwd(torch.zeros(1, 4, 4, 6), wf, 8),            # C % 4
        lambda: K.conv_s2_fwd(x, wf, 6),                                  # Co % 4
        lambda: K.conv_s2_dgrad(dy, wf, 1, 0, 4, 8, 8),                   # H < 1
        lambda: K.conv_s2_fwd(x.double(), wf, 8),                         # dtype
        lambda: K.conv_s2_fwd(x.permute(0, 2, 1, 3), wf, 8),              # contiguity
        lambda: K.conv_s2_wgrad(dy, x, 8, 9, out),                        # more real channels than stored
        lambda: K.conv1x1_s2_wgrad(dy, x, 8, 4, out[:32]),                # the 1x1 needs Ci == C
        lambda: K.conv1x1_s2_dgrad(dy, torch.zeros(8, 4, 1, 1), 1, 4, 4, 8, 8),
        lambda: K.conv_s2_dgrad(dy, wf, 1 << 14, 1 << 8, 1 << 8, 8, 8),   # an operand of 2 GiB or more
    )
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")


@pytest.mark.parametrize("ks", (3, 1))
def test_parity_class_decomposition(ks):
    """dx restricted to the class (ph, pw) of input pixels is the dense product of that class's taps: ky = 1 for an
    even row, ky in {0, 2} for an odd one (reading dy rows i + 1, i), likewise kx; the 1x1 has its tap on the (even,
    even) class only."""
    N, H, W, Ci, Co = 2, 5, 7, 4, 8
    dy = X.ints((N, (H + 1) // 2, (W + 1) // 2, Co), -3, 3, 1)
    w = X.ints((Co, Ci, ks, ks), -2, 2, 2)
    x = torch.zeros(N, Ci, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=2, padding=ks // 2)
    dx = torch.autograd.grad(y, x, dy.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    dyp = F.pad(dy, (0, 0, 0, 1, 0, 1))  # one zero row / column past the end: the shifted reads of odd pixels
    for ph in (0, 1):
        for pw in (0, 1):
            Hc, Wc = (H - ph + 1) // 2, (W - pw + 1) // 2
            want = torch.zeros(N, Hc, Wc, Ci, dtype=torch.float64)
            taps_y = ((1, 0),) if not ph else ((0, 1), (2, 0))  # (ky, shift of the dy row)
            taps_x = ((1, 0),) if not pw else ((0, 1), (2, 0))
            for ky, da in taps_y:
                for kx, db in taps_x:
                    if ks == 3:
                        want += dyp[:, da:da + Hc, db:db + Wc] @ w[:, :, ky, kx]
                    elif not (ph or pw):
                        want += dyp[:, :Hc, :Wc] @ w[:, :, 0, 0]
            assert torch.equal(dx[:, ph::2, pw::2], want), (ks, ph, pw)
