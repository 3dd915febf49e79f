"""Mixup / CutMix in the augment launch: ``ddpx_augment_mix`` equals the CPU twin bit for bit (pixels, labels,
second labels, label weights), a no-mix batch is the plain kernel's batch, and the device-cursor entry point
equals ``make_batch`` eagerly and from a captured graph."""
import pytest
import torch

from ddpx.data.mix import MIX_CUTMIX, MIX_MIXUP, MIX_NONE, MixConfig, Mixer

pytestmark = pytest.mark.gpu

# the configurations and augmentation seeds of tests/test_mix_cpu.py: over them every kind of batch occurs
CONFIGS = {"mixup": MixConfig(0.2, 0.0), "cutmix": MixConfig(0.0, 1.0), "both": MixConfig(0.2, 1.0),
           "half": MixConfig(0.2, 1.0, prob=0.5)}
SEEDS = [0, 1, 2, 3, 4, 5, 690]


def _kind(d):
    if d.mode != MIX_CUTMIX:
        return {MIX_NONE: "none", MIX_MIXUP: "mixup"}[d.mode]
    y0, y1, x0, x1 = d.box
    if (y1 - y0) * (x1 - x0) == 0:
        return "cutmix_empty"
    clipped = y1 - y0 < 2 * (d.cut[0] // 2) or x1 - x0 < 2 * (d.cut[1] // 2)
    return "cutmix_clipped" if clipped else "cutmix_inside"


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(9)
    images = torch.randint(0, 256, (96, 3, 32, 32), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (96,), dtype=torch.int64, generator=g)
    return images, labels, torch.randperm(96, generator=g)


@pytest.mark.parametrize("B", [5, 64])
@pytest.mark.parametrize("layout", ["flat_bf16", "nhwc8_bf16", "nhwc4_f32", "nchw_f32", "nhwc_bf16", "nhwc_f32"])
def test_mixing_augment_matches_cpu_twin(gpu, data, layout, B):
    from ddpx.data.loader import augment_cpu, augment_gpu
    images, labels, perm = data
    gi, gl = images.to(gpu), labels.to(gpu)
    idx = perm[:B].clone()
    idx[-1] = idx[0]  # a repeated image
    seen = set()
    for name, cfg in CONFIGS.items():
        mixer = Mixer(cfg, 32, 32)
        for seed in SEEDS:
            d = mixer.draw(seed)
            seen.add(_kind(d))
            ex, ey, eb, el = augment_cpu(images, labels, idx, seed, True, 4, layout, mix=mixer)
            x, y, tb, lam = augment_gpu(gi, gl, idx.to(gpu), seed, True, 4, layout, mix=mixer)
            assert torch.equal(x.cpu(), ex), (name, seed)
            assert torch.equal(y.cpu(), ey) and torch.equal(tb.cpu(), eb), (name, seed)
            assert lam.dtype == torch.float32 and torch.equal(lam.cpu(), el), (name, seed)
            if d.mode == MIX_NONE:  # the plain kernel's bits
                px, py = augment_gpu(gi, gl, idx.to(gpu), seed, True, 4, layout)
                assert torch.equal(x, px) and torch.equal(y, py), (name, seed)
                assert torch.equal(lam, torch.ones_like(lam))
    assert seen >= {"mixup", "cutmix_clipped", "cutmix_empty", "none"}, seen


def test_tiny_images_take_the_per_thread_parameter_path(gpu):
    # 8x8 images: more than 8 samples per workgroup, so no shared parameter table in LDS
    from ddpx.data.loader import augment_cpu, augment_gpu
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (40, 3, 8, 8), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (40,), dtype=torch.int64, generator=g)
    idx = torch.randperm(40, generator=g)[:37]
    for name in ("both", "half"):
        mixer = Mixer(CONFIGS[name], 8, 8)
        for layout in ("flat_bf16", "nhwc8_bf16"):
            for seed in SEEDS:
                ex, ey, eb, el = augment_cpu(images, labels, idx, seed, True, 2, layout, mix=mixer)
                x, y, tb, lam = augment_gpu(images.to(gpu), labels.to(gpu), idx.to(gpu), seed, True, 2, layout,
                                            mix=mixer)
                assert torch.equal(x.cpu(), ex) and torch.equal(y.cpu(), ey), (name, layout, seed)
                assert torch.equal(tb.cpu(), eb) and torch.equal(lam.cpu(), el), (name, layout, seed)


@pytest.mark.parametrize("layout", ["flat_bf16", "nhwc8_bf16", "nchw_f32"])
def test_mixing_cursor_batch_matches_make_batch(gpu, layout):
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader
    from ddpx.data.sampler import DistributedIndexSampler
    ds = synthetic_cifar(1024, seed=3)
    bs = 128

    def mk():
        return DeviceLoader(ds, bs, gpu, sampler=DistributedIndexSampler(len(ds), 1, 0, shuffle=True, seed=0),
                            train=True, layout=layout, seed=0, mix=MixConfig(0.2, 1.0, prob=0.7))
    loader, ref = mk(), mk()  # (two loaders: each owns its soft-target buffers)
    st, rst = loader.soft_targets, ref.soft_targets
    idx_all = loader._epoch_indices()
    nfull = idx_all.numel() // bs
    idx_dev = idx_all[:nfull * bs].contiguous()
    x0, y0 = ref.make_batch(idx_all[:bs], 0)
    sx, sy = torch.empty_like(x0), torch.empty_like(y0)
    modes = set()

    def check(k):
        b = k % nfull
        ex, ey = ref.make_batch(idx_all[b * bs:(b + 1) * bs], k)
        assert torch.equal(sx, ex) and torch.equal(sy, ey), k
        assert torch.equal(st.tgt_b, rst.tgt_b) and torch.equal(st.lam, rst.lam), k
        assert torch.equal(st.tgt_b, sy.flip(0)), k
        d = ref.mixer.draw(ref.batch_seed(k))
        assert st.lam[0].item() == float(d.wlam), k
        modes.add(d.mode)

    for k in range(nfull + 2):  # wraps around the epoch
        loader.cursor_batch(idx_dev, nfull, sx, sy)
        check(k)
    assert int(loader._cursor.item()) == nfull + 2
    counter = torch.full((1,), nfull + 2, dtype=torch.int32, device=gpu)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            loader.cursor_batch(idx_dev, nfull, sx, sy, counter=counter)
            counter.add_(1)
    torch.cuda.current_stream().wait_stream(s)
    for k in range(nfull + 2, nfull + 5):
        g.replay()
        check(k)
    assert modes == {MIX_NONE, MIX_MIXUP, MIX_CUTMIX}, modes
