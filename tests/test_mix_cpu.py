"""Mixup / CutMix on the CPU: the Beta quantile table, the mixing ``augment_cpu`` against a naive per-pixel loop,
the no-mix identity with the plain ``augment_cpu``, labels and label weights, the loader's persistent
soft-target buffers, and ``singlegpu.py`` with the three flags."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ddpx.data.datasets import synthetic_cifar
from ddpx.data.loader import DeviceLoader, augment_cpu, crop_flip_params
from ddpx.data.mix import BINS, MIX_CUTMIX, MIX_MIXUP, MIX_NONE, MixConfig, Mixer, beta_quantiles, build_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mixup only, cutmix only, both, both with prob 0.5 -- and augmentation seeds chosen so that, over these
# configurations, every kind of batch occurs (asserted below)
CONFIGS = {"mixup": MixConfig(0.2, 0.0), "cutmix": MixConfig(0.0, 1.0), "both": MixConfig(0.2, 1.0),
           "half": MixConfig(0.2, 1.0, prob=0.5)}
SEEDS = [0, 1, 2, 3, 4, 5, 690]


def kind_of(mixer, d):
    if d.mode == MIX_NONE:
        return "none"
    if d.mode == MIX_MIXUP:
        return "mixup"
    y0, y1, x0, x1 = d.box
    if (y1 - y0) * (x1 - x0) == 0:
        return "cutmix_empty"
    clipped = y1 - y0 < 2 * (d.cut[0] // 2) or x1 - x0 < 2 * (d.cut[1] // 2)  # the border cut some of it off
    return "cutmix_clipped" if clipped else "cutmix_inside"


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_quantile_table(alpha):
    q = beta_quantiles(alpha)
    assert q.shape == (BINS,) and q.dtype == np.float64
    assert np.all(np.diff(q) >= 0) and np.all(np.diff(q[::8]) > 0)
    assert abs(q.mean() - 0.5) < 1.0 / BINS
    # symmetric about 1/2 to within one bin: 1 - q[i] lies between the neighbours of q[BINS - 1 - i]
    m = 1.0 - q[::-1]
    assert np.all(m[1:-1] >= q[:-2]) and np.all(m[1:-1] <= q[2:])
    if alpha == 1.0:  # uniform: the quantiles are the bin midpoints
        assert np.allclose(q, (np.arange(BINS) + 0.5) / BINS, atol=1e-9)
    t = build_table(MixConfig(alpha, alpha), 32, 32)
    for row in (0, 1):
        lam = t["lam"][row]
        assert lam.dtype == np.float32 and np.all(lam > 0) and np.all(lam <= 1) and np.all(np.diff(lam) >= 0)
    assert not t["cut_h"][0].any() and not t["cut_w"][0].any()  # Mixup rows: zero box
    assert np.array_equal(t["cut_h"][1], (32 * np.sqrt(1.0 - q)).astype(np.int32))
    assert t.tobytes().__len__() == 2 * BINS * 12


def test_quantiles_match_a_closed_form():
    # Beta(2, 2): F(x) = 3 x^2 - 2 x^3
    q = beta_quantiles(2.0)
    p = (np.arange(BINS) + 0.5) / BINS
    assert np.max(np.abs(3 * q ** 2 - 2 * q ** 3 - p)) < 1e-6
    # Beta(1/2, 1/2) (arcsine): F(x) = 2 / pi asin(sqrt(x))
    q = beta_quantiles(0.5)
    assert np.max(np.abs(2 / np.pi * np.arcsin(np.sqrt(q)) - p)) < 1e-6


def _data(n=16, C=3, H=8, W=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (n, C, H, W), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int64, generator=g)
    return images, labels


def _naive(images, labels, idx, seed, pad, mixer):
    """One pixel at a time, in numpy fp32: crop / flip of the sample and of its partner, then the mix."""
    B = idx.numel()
    _, C, H, W = images.shape
    dy, dx, flip = (t.tolist() for t in crop_flip_params(seed, B, pad))
    d = mixer.draw(seed)
    img = images.numpy()
    inv = np.float32(1.0 / 255.0)

    def pixel(b, c, y, x):
        sy = y + dy[b] - pad
        sx = ((W - 1 - x) if flip[b] else x) + dx[b] - pad
        if not (0 <= sy < H and 0 <= sx < W):
            return np.float32(0.0)
        return np.float32(img[int(idx[b]), c, sy, sx]) * inv

    out = np.zeros((B, C, H, W), dtype=np.float32)
    y0, y1, x0, x1 = d.box
    for b in range(B):
        pb = B - 1 - b
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    va = pixel(b, c, y, x)
                    if d.mode == MIX_MIXUP:
                        va = np.float32(d.lam * va) + np.float32(d.oml * pixel(pb, c, y, x))
                    elif d.mode == MIX_CUTMIX and y0 <= y < y1 and x0 <= x < x1:
                        va = pixel(pb, c, y, x)
                    out[b, c, y, x] = va
    if d.mode == MIX_CUTMIX:
        lam = np.float32(1.0) - np.float32((y1 - y0) * (x1 - x0)) / np.float32(H * W)
    else:
        lam = np.float32(d.lam) if d.mode == MIX_MIXUP else np.float32(1.0)
    return torch.from_numpy(out), labels[idx], labels[idx.flip(0)], torch.full((B,), float(lam)), d


def test_mixing_augment_cpu_matches_naive_loop():
    images, labels = _data()
    idx = torch.tensor([7, 3, 11, 3, 0])  # B = 5: the middle sample is its own partner; a repeated image
    seen = set()
    for name, cfg in CONFIGS.items():
        mixer = Mixer(cfg, 8, 8)
        for seed in SEEDS:
            ex, ey, eb, el, d = _naive(images, labels, idx, seed, 2, mixer)
            seen.add(kind_of(mixer, d))
            x, y, tb, lam = augment_cpu(images, labels, idx, seed, True, 2, "nchw_f32", mix=mixer)
            assert torch.equal(x, ex), (name, seed)
            assert torch.equal(y, ey) and torch.equal(tb, eb) and torch.equal(tb, y.flip(0)), (name, seed)
            assert lam.dtype == torch.float32 and torch.equal(lam, el), (name, seed)
            plain_x, plain_y = augment_cpu(images, labels, idx, seed, True, 2, "nchw_f32")
            # (Beta(0.2, 0.2)'s top quantiles round to lam = 1 in fp32: a Mixup batch that changes nothing)
            if d.mode == MIX_NONE or kind_of(mixer, d) == "cutmix_empty" or float(d.wlam) == 1.0:
                assert torch.equal(x, plain_x) and float(lam[0]) == 1.0, (name, seed)
            else:
                assert not torch.equal(x, plain_x), (name, seed)
            if d.mode == MIX_CUTMIX:
                y0, y1, x0, x1 = d.box
                assert float(lam[0]) == float(np.float32(1) - np.float32((y1 - y0) * (x1 - x0)) / np.float32(64))
                outside = torch.ones(8, 8, dtype=torch.bool)
                outside[y0:y1, x0:x1] = False
                assert torch.equal(x[:, :, outside], plain_x[:, :, outside])
                assert torch.equal(x[:, :, ~outside], plain_x.flip(0)[:, :, ~outside])
    assert seen >= {"mixup", "cutmix_clipped", "cutmix_empty", "none"}, seen


@pytest.mark.parametrize("layout", ["nchw_f32", "nchw_bf16", "flat_bf16", "nhwc_bf16", "nhwc_f32", "nhwc8_bf16",
                                    "nhwc4_f32"])
def test_layouts_and_no_mix_identity(layout):
    images, labels = _data()
    idx = torch.tensor([7, 3, 11, 3, 0])
    half = Mixer(CONFIGS["half"], 8, 8)
    kinds = set()
    for seed in SEEDS:
        d = half.draw(seed)
        kinds.add(d.mode)
        x, y, tb, lam = augment_cpu(images, labels, idx, seed, True, 2, layout, mix=half)
        px, py = augment_cpu(images, labels, idx, seed, True, 2, layout)
        assert x.shape == px.shape and x.dtype == px.dtype and torch.equal(y, py)
        if d.mode == MIX_NONE:
            assert torch.equal(x, px) and torch.equal(lam, torch.ones(5))
        # every layout is the NCHW fp32 batch, permuted / padded / rounded
        ref = augment_cpu(images, labels, idx, seed, True, 2, "nchw_f32", mix=half)[0]
        back = x.float()
        if layout.startswith("nhwc"):
            back = back[..., :3].permute(0, 3, 1, 2)
        want = ref.to(x.dtype).float() if "bf16" in layout else ref
        assert torch.equal(back.reshape(ref.shape), want), (layout, seed)
    assert kinds == {MIX_NONE, MIX_MIXUP, MIX_CUTMIX}
    # mix=None and evaluation batches: the present function, unchanged
    assert len(augment_cpu(images, labels, idx, 3, True, 2, layout, mix=None)) == 2
    ev = augment_cpu(images, labels, idx, 3, False, 2, layout, mix=half)
    assert len(ev) == 2 and torch.equal(ev[0], augment_cpu(images, labels, idx, 3, False, 2, layout)[0])


def test_loader_soft_target_buffers_and_determinism():
    ds = synthetic_cifar(100, seed=1)
    cfg = MixConfig(0.2, 1.0)
    mk = lambda **kw: DeviceLoader(ds, 32, "cpu", train=True, layout="flat_f32", seed=5, **kw)  # noqa: E731
    a, b, plain = mk(mix=cfg), mk(mix=cfg), mk()
    assert plain.soft_targets is None and mk(mix=MixConfig()).soft_targets is None
    assert DeviceLoader(ds, 32, "cpu", train=False, mix=cfg).soft_targets is None  # evaluation never mixes
    st = a.soft_targets
    assert st.tgt_b.shape == (32,) and st.lam.shape == (32,) and st.label_smoothing == 0.0
    ptrs = (st.tgt_b.data_ptr(), st.lam.data_ptr())
    for ld in (a, b, plain):
        ld.set_epoch(2)
    mixed_any = False
    for step, ((xa, ya), (xb, yb), (xp, yp)) in enumerate(zip(a, b, plain)):
        n = xa.shape[0]  # 32, 32, 32, 4: the partial batch writes a prefix
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ya, yp)
        assert torch.equal(st.tgt_b[:n], ya.flip(0)) and torch.equal(st.tgt_b, b.soft_targets.tgt_b)
        assert torch.equal(st.lam, b.soft_targets.lam)
        d = a.mixer.draw(a.batch_seed(step))
        assert float(st.lam[0]) == float(d.wlam) and bool((st.lam[:n] == st.lam[0]).all())
        assert torch.equal(xa, xp) == (d.mode == MIX_NONE or float(d.wlam) == 1.0)
        mixed_any |= d.mode != MIX_NONE
    assert step == 3 and n == 4 and mixed_any
    assert ptrs == (st.tgt_b.data_ptr(), st.lam.data_ptr())  # persistent: a captured step may hold them


def test_singlegpu_cli_with_all_three_flags(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "singlegpu.py"), "1", "1", "--device", "cpu", "--model", "mlp", "--data",
           "synthetic", "--hidden", "128", "--batch_size", "64", "--train_size", "256", "--test_size", "64",
           "--label_smoothing", "0.1", "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0", "--metrics", "m.jsonl"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert re.search(r"fp32 model has accuracy=\d+\.\d\d%", r.stdout)
    import json
    recs = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    losses = [rec["loss"] for rec in recs if "epoch" in rec]
    assert len(losses) == 1 and np.isfinite(losses[0]) and losses[0] > 0
