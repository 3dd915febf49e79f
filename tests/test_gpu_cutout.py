"""Cutout inside the augment launch: the GPU batch equals the CPU twin bit for bit in all six layouts, plain and with
Mixup / CutMix / a "no mix" draw, through the cursor entry points too; ``cutout=0`` is the launch without the
argument; labels, second labels and ``lam`` are untouched."""
import pytest
import torch

from ddpx.data.mix import MIX_CUTMIX, MIX_MIXUP, MIX_NONE, MixConfig, Mixer

pytestmark = pytest.mark.gpu

LAYOUTS = ["flat_bf16", "nhwc8_bf16", "nhwc4_f32", "nchw_f32", "nhwc_bf16", "nhwc_f32"]
# Mixup only, CutMix only, and a configuration that leaves half of the batches unmixed
MIXES = {"mixup": (MixConfig(0.2, 0.0), MIX_MIXUP), "cutmix": (MixConfig(0.0, 1.0), MIX_CUTMIX),
         "none": (MixConfig(0.2, 1.0, prob=0.5), MIX_NONE)}


def _data(size, n=24, height=None):
    g = torch.Generator().manual_seed(size)
    images = torch.randint(1, 256, (n, 3, height or size, size), dtype=torch.uint8, generator=g)  # no zero pixel
    labels = torch.randint(0, 10, (n,), dtype=torch.int64, generator=g)
    return images, labels, torch.randperm(n, generator=g)


def _seed_with(mixer, mode, start):
    """The first augmentation seed >= start whose batch draw has the wanted mode."""
    for seed in range(start, start + 200):
        if mixer.draw(seed).mode == mode:
            return seed
    raise AssertionError("no such draw in 200 seeds")


@pytest.mark.parametrize("B", [5, 8])
@pytest.mark.parametrize("size,S", [(16, 5), (32, 8), (8, 3)], ids=["16x16", "32x32", "8x8"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cutout_matches_cpu_twin(gpu, layout, size, S, B):
    """B = 5: the middle sample is its own partner.  W == 32 is gather_row8's own path.  With at most 8 samples in the
    batch every workgroup here reads the parameters from its LDS block (the per-thread draw: the test below)."""
    _check_against_twin(gpu, layout, _data(size), S, B)


def _samples_per_workgroup(layout, H, W, B, C=3):
    """The most samples a 256-thread workgroup of the augment kernels touches (``nb`` there)."""
    per = H * W if layout.startswith("nhwc") else C * H * (W // 8)  # threads per sample
    total = B * per
    return max(min(total, t0 + 256) // per - t0 // per + (min(total, t0 + 256) % per != 0)
               for t0 in range(0, total, 256))


@pytest.mark.parametrize("H,W,S", [(8, 8, 3), (2, 8, 3)], ids=["8x8", "2x8"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cutout_on_the_per_thread_parameter_path(gpu, layout, H, W, S):
    """More than 8 samples in one workgroup: no LDS parameter block, every thread draws its own crop, flip and Cutout
    centre (and its partner's).  B = 24: at 8x8 the NCHW / flat layouts have 24 threads per sample (11 samples in a
    workgroup); the NHWC layouts have H * W threads per sample and need the 2x8 images (16 samples in a workgroup)."""
    B = 24
    nb = _samples_per_workgroup(layout, H, W, B)
    if layout.startswith("nhwc") and (H, W) == (8, 8):
        assert nb <= 8  # 4 samples in a workgroup: the LDS block again, kept as one more case of it
    else:
        assert nb > 8, nb
    _check_against_twin(gpu, layout, _data(W, height=H), S, B)


def _check_against_twin(gpu, layout, data, S, B):
    from ddpx.data.loader import augment_cpu, augment_gpu
    images, labels, perm = data
    size = images.shape[-1]
    H = images.shape[-2]
    gi, gl = images.to(gpu), labels.to(gpu)
    idx = perm[:B].clone()
    gidx = idx.to(gpu)
    for seed in (3, 11):
        ex, ey = augment_cpu(images, labels, idx, seed, True, 2, layout, cutout=S)
        x, y = augment_gpu(gi, gl, gidx, seed, True, 2, layout, cutout=S)
        assert torch.equal(x.cpu(), ex) and torch.equal(y.cpu(), ey), seed
        px, py = augment_gpu(gi, gl, gidx, seed, True, 2, layout)
        assert torch.equal(y, py) and not torch.equal(x, px), seed  # something was erased; labels unchanged
        zx, zy = augment_gpu(gi, gl, gidx, seed, True, 2, layout, cutout=0)
        assert torch.equal(zx, px) and torch.equal(zy, py), seed
        evx, _ = augment_gpu(gi, gl, gidx, seed, False, 2, layout, cutout=S)  # evaluation batches are never erased
        assert torch.equal(evx, augment_gpu(gi, gl, gidx, seed, False, 2, layout)[0]), seed
    for name, (cfg, mode) in MIXES.items():
        mixer = Mixer(cfg, H, size)
        seed = _seed_with(mixer, mode, 5)
        ex, ey, eb, el = augment_cpu(images, labels, idx, seed, True, 2, layout, mix=mixer, cutout=S)
        x, y, tb, lam = augment_gpu(gi, gl, gidx, seed, True, 2, layout, mix=mixer, cutout=S)
        assert torch.equal(x.cpu(), ex), (name, seed)
        assert torch.equal(y.cpu(), ey) and torch.equal(tb.cpu(), eb) and torch.equal(lam.cpu(), el), (name, seed)
        # labels, second labels and lam are the uncut launch's; cutout = 0 is that launch
        px, py, pb, pl = augment_gpu(gi, gl, gidx, seed, True, 2, layout, mix=mixer)
        assert torch.equal(y, py) and torch.equal(tb, pb) and torch.equal(lam, pl), (name, seed)
        zx, _, _, _ = augment_gpu(gi, gl, gidx, seed, True, 2, layout, mix=mixer, cutout=0)
        assert torch.equal(zx, px) and not torch.equal(x, px), (name, seed)
        if mode == MIX_NONE:  # a "no mix" draw writes the plain kernel's bits, Cutout included
            assert torch.equal(x, augment_gpu(gi, gl, gidx, seed, True, 2, layout, cutout=S)[0]), seed


def test_erased_pixels_are_the_stated_squares(gpu):
    """On an all-255 image without a crop border the zeros of the GPU batch are the twin's rectangles."""
    from ddpx.data.loader import augment_gpu, cutout_params
    from tests._tail_ref import cutout_box
    B, H = 16, 32
    images = torch.full((B, 3, H, H), 255, dtype=torch.uint8, device=gpu)
    labels = torch.zeros(B, dtype=torch.int64, device=gpu)
    x, _ = augment_gpu(images, labels, torch.arange(B, device=gpu), 4242, True, 0, "nchw_f32", cutout=8)
    cy, cx = cutout_params(4242, B, H, H)
    for b in range(B):
        y0, y1, x0, x1 = cutout_box(int(cy[b]), int(cx[b]), 8, H, H)
        want = torch.ones(3, H, H)
        want[:, y0:y1, x0:x1] = 0.0
        assert torch.equal(x[b].cpu(), want), b


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("layout", ["nhwc8_bf16", "flat_bf16", "nchw_f32"])
def test_cursor_entry_points(gpu, layout, mixed):
    """``ddpx_augment_cursor`` / ``ddpx_augment_mix_cursor`` with Cutout at cursor values 0 and 3."""
    from ddpx.data.datasets import synthetic_cifar
    from ddpx.data.loader import DeviceLoader, augment_cpu
    from ddpx.data.sampler import DistributedIndexSampler
    ds = synthetic_cifar(64, seed=3)
    bs = 8
    loader = DeviceLoader(ds, bs, gpu, sampler=DistributedIndexSampler(len(ds), 1, 0, shuffle=True, seed=0),
                          train=True, layout=layout, seed=0, cutout=8,
                          mix=MixConfig(0.2, 1.0, prob=0.7) if mixed else None)
    assert loader.cutout == 8
    idx_all = loader._epoch_indices()
    nfull = idx_all.numel() // bs
    x0, y0 = loader.make_batch(idx_all[:bs], 0)
    sx, sy = torch.empty_like(x0), torch.empty_like(y0)
    images, labels = ds.images.cpu(), ds.labels.cpu()
    for k in (0, 3):
        counter = torch.full((1,), k, dtype=torch.int32, device=gpu)
        loader.cursor_batch(idx_all, nfull, sx, sy, counter=counter)
        idx = idx_all[(k % nfull) * bs:(k % nfull + 1) * bs].cpu()
        want = augment_cpu(images, labels, idx, loader.batch_seed(k), True, loader.pad, layout, mix=loader.mixer,
                           cutout=8)
        assert torch.equal(sx.cpu(), want[0]) and torch.equal(sy.cpu(), want[1]), k
        if mixed:
            st = loader.soft_targets
            assert torch.equal(st.tgt_b.cpu(), want[2]) and torch.equal(st.lam.cpu(), want[3]), k
        ex, ey = loader.make_batch(idx_all[(k % nfull) * bs:(k % nfull + 1) * bs], k)
        assert torch.equal(sx, ex) and torch.equal(sy, ey), k
        assert int(counter.item()) == k  # read, not advanced


def test_entry_points_bound_the_side(gpu):
    from ddpx.data.loader import LAYOUTS as CODES
    from ddpx.runtime import native
    lib = native.kernels()
    B, H = 4, 32
    images = torch.zeros(B, 3, H, H, dtype=torch.uint8, device=gpu)
    labels = torch.zeros(B, dtype=torch.int64, device=gpu)
    idx = torch.arange(B, device=gpu)
    out = torch.full((B, 3, H, H), -1.0, device=gpu)
    tgt = torch.zeros(B, dtype=torch.int64, device=gpu)
    cur = torch.zeros(1, dtype=torch.int32, device=gpu)
    s = native.stream_handle()

    def plain(S):
        return lib.ddpx_augment(images.data_ptr(), labels.data_ptr(), idx.data_ptr(), B, 3, H, H, 4, 1, 1, S,
                                CODES["nchw_f32"], out.data_ptr(), tgt.data_ptr(), s)

    def cursor(S):
        return lib.ddpx_augment_cursor(images.data_ptr(), labels.data_ptr(), idx.data_ptr(), 1, B, 3, H, H, 4, 1, 1, S,
                                       CODES["nchw_f32"], out.data_ptr(), tgt.data_ptr(), cur.data_ptr(), s)

    for fn in (plain, cursor):
        assert fn(-1) == -7 and fn(2 * H + 1) == -7
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was launched
    assert plain(2 * H) == 0 and cursor(0) == 0
