"""Cutout on the CPU twin: the draw against a scalar Python re-implementation, the erased rectangle on an all-255
image, and the untouched default."""
import pytest
import torch

from tests import _tail_ref as T


def _data(n, H, W, value=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    if value is None:
        images = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)
    else:
        images = torch.full((n, 3, H, W), value, dtype=torch.uint8)
    return images, torch.randint(0, 10, (n,), generator=g)


@pytest.mark.parametrize("H,W", [(32, 32), (16, 16), (8, 24)])
def test_cutout_params_equal_the_scalar_draw(H, W):
    from ddpx.data import loader as L
    for seed in (0, 12345, (1 << 63) + 17):
        cy, cx = L.cutout_params(seed, 9, H, W)
        want = T.cutout_params_scalar(seed, 9, H, W, L._CUT_SALT)
        assert list(zip(cy.tolist(), cx.tolist())) == want
        assert all(0 <= a < H and 0 <= b < W for a, b in want)
    assert L._CUT_SALT % 2 == 1 and L._CUT_SALT != 0x8CB92BA72F3D8DD7 and L._CUT_SALT < 1 << 64


@pytest.mark.parametrize("S", [8, 5, 1, 64])
def test_zeros_are_exactly_the_stated_rectangle(S):
    """All-255 image, pad = 0 (no crop border): the zeros of every sample are rows [cy - S // 2, cy - S // 2 + S)
    x the same columns, cut off at the border.  S = 2H erases everything.  Many samples: centres on the border
    (cy or cx in {0, H - 1}) are among them."""
    from ddpx.data.loader import augment_cpu, cutout_params
    H = W = 32
    B = 64
    images, labels = _data(B, H, W, value=255)
    idx = torch.arange(B)
    seed = 4242
    x, y = augment_cpu(images, labels, idx, seed, True, 0, "nchw_f32", cutout=S)
    assert torch.equal(y, labels)
    cy, cx = cutout_params(seed, B, H, W)
    border = 0
    for b in range(B):
        y0, y1, x0, x1 = T.cutout_box(int(cy[b]), int(cx[b]), S, H, W)
        want = torch.ones(3, H, W)
        want[:, y0:y1, x0:x1] = 0.0
        assert torch.equal(x[b], want), (b, int(cy[b]), int(cx[b]))
        border += int(cy[b]) in (0, H - 1) or int(cx[b]) in (0, W - 1)
        if S == 64:
            assert not x[b].any()
        if S == 1:
            assert int((x[b] == 0).sum()) == 3
    assert border > 0  # the case list holds centres on the border


def test_border_boxes_are_cut_off_not_shifted():
    assert T.cutout_box(0, 0, 8, 32, 32) == (0, 4, 0, 4)
    assert T.cutout_box(31, 31, 8, 32, 32) == (27, 32, 27, 32)
    assert T.cutout_box(0, 31, 5, 32, 32) == (0, 3, 29, 32)
    assert T.cutout_box(16, 16, 64, 32, 32) == (0, 32, 0, 32)


@pytest.mark.parametrize("layout", ["nchw_f32", "nhwc8_bf16", "flat_bf16"])
def test_cutout_zero_is_the_plain_batch_and_eval_never_erases(layout):
    from ddpx.data.loader import augment_cpu
    images, labels = _data(12, 32, 32, seed=3)
    idx = torch.randperm(12)
    plain = augment_cpu(images, labels, idx, 77, True, 4, layout)
    zero = augment_cpu(images, labels, idx, 77, True, 4, layout, cutout=0)
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
    cut = augment_cpu(images, labels, idx, 77, True, 4, layout, cutout=8)
    assert not torch.equal(plain[0], cut[0]) and torch.equal(plain[1], cut[1])
    ev = augment_cpu(images, labels, idx, 77, False, 4, layout)
    assert torch.equal(ev[0], augment_cpu(images, labels, idx, 77, False, 4, layout, cutout=8)[0])


def test_cutout_comes_after_crop_and_flip_and_before_the_mix():
    """Output coordinates: the erased square sits at the same place whatever the crop and flip did; with Mixup the
    partner's pixels carry the partner's own square, and labels / lam are the uncut batch's."""
    from ddpx.data.loader import augment_cpu, cutout_params
    from ddpx.data.mix import MixConfig, Mixer
    images, labels = _data(5, 32, 32, value=255)
    idx = torch.arange(5)
    seed, S = 99, 8
    x, _ = augment_cpu(images, labels, idx, seed, True, 4, "nchw_f32", cutout=S)
    cy, cx = cutout_params(seed, 5, 32, 32)
    for b in range(5):
        y0, y1, x0, x1 = T.cutout_box(int(cy[b]), int(cx[b]), S, 32, 32)
        assert not x[b, :, y0:y1, x0:x1].any()
    mixer = Mixer(MixConfig(1.0, 0.0, 1.0, 0.5), 32, 32)  # Mixup on every batch
    mx, my, mb, ml = augment_cpu(images, labels, idx, seed, True, 4, "nchw_f32", mix=mixer, cutout=S)
    px, py, pb, pl = augment_cpu(images, labels, idx, seed, True, 4, "nchw_f32", mix=mixer)
    assert torch.equal(my, py) and torch.equal(mb, pb) and torch.equal(ml, pl)
    d = mixer.draw(seed)
    want = float(d.lam) * x + float(d.oml) * x.flip(0)
    assert torch.equal(mx, want)
    # the middle sample is its own partner: its square is erased outright
    y0, y1, x0, x1 = T.cutout_box(int(cy[2]), int(cx[2]), S, 32, 32)
    assert not mx[2, :, y0:y1, x0:x1].any()


def test_bad_sizes_raise():
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader, augment_cpu
    images, labels = _data(4, 32, 32)
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            augment_cpu(images, labels, torch.arange(4), 1, True, 4, "nchw_f32", cutout=bad)
        with pytest.raises(ValueError):
            DeviceLoader(synthetic_cifar(8, seed=0), 4, "cpu", cutout=bad)
    assert DeviceLoader(synthetic_cifar(8, seed=0), 4, "cpu", train=False, cutout=8).cutout == 0
    assert DeviceLoader(synthetic_cifar(8, seed=0), 4, "cpu", cutout=8).cutout == 8
