"""Host-side shape logic of the stride-2 convolution wrappers (ddpx/ops/conv.py): output sizes and the argument
errors raised before any library call."""
import pytest
import torch

from ddpx.ops import conv as K

BF16 = torch.bfloat16


@pytest.mark.parametrize("hw,want", [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((1, 8), (1, 4)), ((3, 5), (2, 3)),
                                     ((7, 7), (4, 4)), ((12, 12), (6, 6)), ((32, 17), (16, 9))])
def test_s2_out_hw_matches_torch(hw, want):
    assert K.s2_out_hw(*hw) == want
    x = torch.zeros(1, 1, *hw)
    for k in (3, 1):
        y = torch.nn.functional.conv2d(x, torch.zeros(1, 1, k, k), stride=2, padding=k // 2)
        assert tuple(y.shape[2:]) == want


def test_s2_argument_errors():
    x = torch.zeros(1, 4, 4, 8, dtype=BF16)
    w3, w1 = torch.zeros(8 * 9 * 8, dtype=BF16), torch.zeros(8 * 8, dtype=BF16)
    dy = torch.zeros(4, 8, dtype=BF16)
    with pytest.raises(ValueError, match="H, W >= 1"):
        K.s2_out_hw(0, 4)
    with pytest.raises(ValueError, match="multiples of 8"):
        K.conv_s2_fwd(torch.zeros(1, 4, 4, 12, dtype=BF16), w3, 8)
    with pytest.raises(ValueError, match="multiples of 8"):
        K.conv1x1_s2_dgrad(dy, w1, 1, 4, 4, 8, 12)
    with pytest.raises(ValueError, match="H, W >= 1"):
        K.conv1x1_s2_fwd(torch.zeros(1, 0, 4, 8, dtype=BF16), w1, 8)
    with pytest.raises(ValueError, match="channel mismatch"):
        K.conv_s2_fwd(x, w1, 8)
    with pytest.raises(ValueError, match=r"dy must be \[N\*Ho\*Wo, Co\]"):
        K.conv_s2_dgrad(dy, w3, 1, 5, 5, 8, 8)  # Ho = Wo = 3: 9 rows, not 4
    with pytest.raises(ValueError, match="exactly one of out and sgd"):
        K.conv_s2_wgrad(dy, x, 8, 8)
    with pytest.raises(ValueError, match="bad out"):
        K.conv1x1_s2_wgrad(dy, x, 8, 8, out=torch.zeros(8 * 8 * 9))
