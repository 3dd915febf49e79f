"""GPU-resident batch loader: sampler indices → gather + augment kernel → batch.

Replaces ``DataLoader(ds, batch_size, pin_memory=True, shuffle|sampler)``
(``/root/reference/singlegpu.py:174-180``, ``multigpu.py:147-154``) and the
blocking per-batch ``.to(gpu_id)`` copies (``singlegpu.py:114-115``).  The uint8
dataset lives on the device once; each batch is produced by ONE kernel
(``ddpx_augment``: gather, RandomCrop(32, pad 4), RandomHorizontalFlip,
ToTensor scaling) directly in the layout the model consumes.

On CPU the same transform runs with vectorised torch indexing and the *same*
counter-based random stream, so CPU and GPU batches are bit-identical (tested).

``len(loader)`` and the last partial batch follow the reference
(``drop_last=False``): 98 steps of 512 (last 336) for 50k samples on one rank.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops.loss import SoftTargets
from ..runtime import native
from .datasets import ImageDataset
from .mix import MIX_CUTMIX, MIX_MIXUP, MixConfig, Mixer
from .sampler import DistributedIndexSampler

LAYOUTS = {"nchw_f32": 0, "nchw_bf16": 1, "nhwc_bf16": 2, "nhwc_f32": 3, "flat_bf16": 1, "flat_f32": 0,
           "nhwc8_bf16": 4, "nhwc4_f32": 5}

_M64 = (1 << 64) - 1


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(_M64)
    x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(_M64)
    x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & np.uint64(_M64)
    return x ^ (x >> np.uint64(31))


def crop_flip_params(seed: int, batch: int, pad: int = 4):
    """(dy, dx, flip) per sample — identical to the HIP kernel's stream."""
    b = np.arange(1, batch + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (np.uint64(seed & _M64) ^ ((np.uint64(0xD1B54A32D192ED03) * b) & np.uint64(_M64)))
        r = _splitmix64_np(key)
    m = np.uint64(2 * pad + 1)
    dy = (r % m).astype(np.int64)
    dx = ((r >> np.uint64(16)) % m).astype(np.int64)
    flip = ((r >> np.uint64(40)) & np.uint64(1)).astype(np.int64)
    return torch.from_numpy(dy), torch.from_numpy(dx), torch.from_numpy(flip)


_CUT_SALT = 0xA0761D6478BD642F  # kCutSalt of csrc/kernels/data_augment.hip


def cutout_params(seed: int, batch: int, H: int, W: int):
    """(cy, cx) per sample: the centres of the Cutout squares, in output coordinates — the HIP kernel's draw:
    ``rc = splitmix64(r ^ SALT)`` with ``r`` the sample's crop / flip hash (:func:`crop_flip_params`),
    ``cy = rc % H``, ``cx = (rc >> 20) % W``."""
    b = np.arange(1, batch + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (np.uint64(seed & _M64) ^ ((np.uint64(0xD1B54A32D192ED03) * b) & np.uint64(_M64)))
        rc = _splitmix64_np(_splitmix64_np(key) ^ np.uint64(_CUT_SALT))
    cy = (rc % np.uint64(H)).astype(np.int64)
    cx = ((rc >> np.uint64(20)) % np.uint64(W)).astype(np.int64)
    return torch.from_numpy(cy), torch.from_numpy(cx)


def _check_cutout(cutout, H, W):
    cutout = int(cutout)
    if not 0 <= cutout <= 2 * max(H, W):
        raise ValueError(f"cutout must lie in 0..{2 * max(H, W)} for {H}x{W} images, got {cutout}")
    return cutout


def augment_cpu(images_u8, labels, idx, seed, train=True, pad=4, layout="nchw_f32", mix: Mixer | None = None,
                cutout: int = 0):
    """The batch as ``ddpx_augment`` writes it.  With ``mix`` (training only) as ``ddpx_augment_mix`` writes it,
    and the return grows to (x, y, tgt_b, lam): the partners' labels and the batch's label weight.

    ``cutout`` = S > 0 (training only): rows [cy - S // 2, cy - S // 2 + S) x the same columns of every sample,
    centre from :func:`cutout_params`, are 0.0 after crop and flip; the image bounds cut the square off.  Each
    sample is erased before the mix, so a partner's pixels carry the partner's own square."""
    x = images_u8[idx]  # [B,C,H,W] uint8
    B, C, H, W = x.shape
    y = labels[idx]
    if train:
        dy, dx, flip = crop_flip_params(seed, B, pad)
        xp = torch.nn.functional.pad(x.float(), (pad, pad, pad, pad))
        rows = dy[:, None] + torch.arange(H)[None, :]                      # [B,H]
        cols = dx[:, None] + torch.arange(W)[None, :]                      # [B,W]
        cols = torch.where(flip[:, None].bool(), cols.flip(1), cols)
        bi = torch.arange(B)[:, None, None, None]
        ci = torch.arange(C)[None, :, None, None]
        out = xp[bi, ci, rows[:, None, :, None], cols[:, None, None, :]]
    else:
        out = x.float()
    out = out * (1.0 / 255.0)  # same fp32 constant multiply as the HIP kernel (bit-identical)
    cutout = _check_cutout(cutout, H, W)
    if cutout and train:
        cy, cx = cutout_params(seed, B, H, W)
        y0, x0 = cy - cutout // 2, cx - cutout // 2
        ys, xs = torch.arange(H)[None, :], torch.arange(W)[None, :]
        in_y = (ys >= y0[:, None]) & (ys < y0[:, None] + cutout)   # [B,H]
        in_x = (xs >= x0[:, None]) & (xs < x0[:, None] + cutout)   # [B,W]
        out = out.masked_fill((in_y[:, :, None] & in_x[:, None, :])[:, None], 0.0)
    mixing = mix is not None and train
    if mixing:
        d = mix.draw(seed)
        partner = out.flip(0)  # sample B - 1 - b, already under its own crop and flip
        if d.mode == MIX_MIXUP:
            # two rounded products and a rounded sum, as the kernel's explicit multiply / add
            out = float(d.lam) * out + float(d.oml) * partner
        elif d.mode == MIX_CUTMIX:
            y0, y1, x0, x1 = d.box
            out = out.clone()
            out[:, :, y0:y1, x0:x1] = partner[:, :, y0:y1, x0:x1]
        tgt_b = y.flip(0)
        lam = torch.full((B,), float(d.wlam), dtype=torch.float32)
    if layout in ("nhwc_bf16", "nhwc_f32", "nhwc8_bf16", "nhwc4_f32"):
        out = out.permute(0, 2, 3, 1).contiguous()
    if layout == "nhwc8_bf16":
        out = torch.nn.functional.pad(out, (0, 8 - C))
    if layout == "nhwc4_f32":
        out = torch.nn.functional.pad(out, (0, 4 - C))
    if layout in ("flat_bf16", "flat_f32"):
        out = out.reshape(B, -1)
    if "bf16" in layout:
        out = out.to(torch.bfloat16)
    if mixing:
        return out, y, tgt_b, lam
    return out, y


def augment_gpu(images_u8, labels, idx, seed, train=True, pad=4, layout="nchw_f32", out=None, tgt=None,
                mix: Mixer | None = None, tgt_b=None, lam=None, cutout: int = 0):
    """One ``ddpx_augment`` launch; with ``mix`` (training only) one ``ddpx_augment_mix`` launch, returning
    (x, y, tgt_b, lam).  ``cutout``: as :func:`augment_cpu`, inside the same launch."""
    B = idx.numel()
    _, C, H, W = images_u8.shape
    cutout = _check_cutout(cutout, H, W)
    code = LAYOUTS[layout]
    dt = torch.bfloat16 if "bf16" in layout else torch.float32
    shape = {"nchw_f32": (B, C, H, W), "nchw_bf16": (B, C, H, W), "nhwc_bf16": (B, H, W, C),
             "nhwc_f32": (B, H, W, C), "flat_bf16": (B, C * H * W), "flat_f32": (B, C * H * W),
             "nhwc8_bf16": (B, H, W, 8), "nhwc4_f32": (B, H, W, 4)}[layout]
    if out is None:
        out = torch.empty(shape, dtype=dt, device=images_u8.device)
    if tgt is None:
        tgt = torch.empty((B,), dtype=torch.int64, device=images_u8.device)
    if out.numel() < B * C * H * W or tgt.numel() < B:
        raise ValueError("augment: output buffers too small")
    if idx.dtype != torch.int64 or not idx.is_cuda:
        raise ValueError("augment: idx must be an int64 device tensor")
    lib = native.kernels()
    if mix is not None and train:
        dev = images_u8.device
        if tgt_b is None:
            tgt_b = torch.empty((B,), dtype=torch.int64, device=dev)
        if lam is None:
            lam = torch.empty((B,), dtype=torch.float32, device=dev)
        _check_mix_buffers(mix, H, W, B, tgt_b, lam)
        rc = lib.ddpx_augment_mix(images_u8.data_ptr(), labels.data_ptr(), idx.data_ptr(), B, C, H, W, pad,
                                  seed & _M64, cutout, code, out.data_ptr(), tgt.data_ptr(),
                                  mix.device_table(dev).data_ptr(), mix.cfg.modes, mix.cfg.p_apply, mix.cfg.p_switch,
                                  tgt_b.data_ptr(), lam.data_ptr(), native.stream_handle())
        native.check(rc, "ddpx_augment_mix")
        return out, tgt, tgt_b[:B], lam[:B]
    rc = lib.ddpx_augment(images_u8.data_ptr(), labels.data_ptr(), idx.data_ptr(), B, C, H, W, pad,
                          seed & _M64, int(train), cutout, code, out.data_ptr(), tgt.data_ptr(),
                          native.stream_handle())
    native.check(rc, "ddpx_augment")
    return out, tgt


def _check_mix_buffers(mix, H, W, B, tgt_b, lam):
    if (mix.H, mix.W) != (H, W):
        raise ValueError("augment: the mixing table was built for another image size")
    if (tgt_b.dtype != torch.int64 or lam.dtype != torch.float32 or tgt_b.numel() < B or lam.numel() < B
            or not tgt_b.is_cuda or not lam.is_cuda):
        raise ValueError("augment: tgt_b / lam must be int64 / fp32 device tensors of >= batch elements")


class DeviceLoader:
    """Iterable of (inputs, targets) batches produced on ``device``."""

    def __init__(self, dataset: ImageDataset, batch_size: int, device, sampler: DistributedIndexSampler | None = None,
                 train: bool = True, layout: str = "nchw_f32", seed: int = 0, pad: int = 4,
                 mix: MixConfig | None = None, cutout: int = 0):
        self.device = torch.device(device)
        self.ds = dataset.to(self.device)
        # Cutout: a training loader erases one square of this side per sample; an evaluation loader never does
        self.cutout = _check_cutout(cutout, *self.ds.images.shape[-2:]) if train else 0
        self.batch_size = batch_size
        self.sampler = sampler or DistributedIndexSampler(len(dataset), 1, 0, shuffle=train, seed=seed)
        self.train = train
        self.layout = layout
        self.seed = seed
        self.pad = pad
        self.epoch = 0
        self._idx = None
        self._idx_epoch = None
        # Mixup / CutMix (training loaders only): every batch also writes the partners' labels and the label
        # weight into these persistent buffers (a partial last batch: their prefix), which the loss reads in
        # place, so a captured step follows them with no re-capture.  Batches stay (x, y).
        self.mixer = None
        self.soft_targets = None
        if mix is not None and mix.enabled and train:
            _, _, H, W = self.ds.images.shape
            self.mixer = Mixer(mix, H, W)
            self.soft_targets = SoftTargets(torch.zeros(batch_size, dtype=torch.int64, device=self.device),
                                            torch.ones(batch_size, dtype=torch.float32, device=self.device))

    def set_epoch(self, epoch: int):
        self.epoch = epoch
        self.sampler.set_epoch(epoch)

    def __len__(self):
        return math.ceil(len(self.sampler) / self.batch_size)

    def _epoch_indices(self):
        if self._idx is None or self._idx_epoch != self.epoch:
            self._idx = self.sampler.indices().to(self.device)
            self._idx_epoch = self.epoch
        return self._idx

    def batch_seed(self, step: int) -> int:
        return (self.seed * 1_000_003 + self.epoch * 65_537 + step) & _M64

    def make_batch(self, idx: torch.Tensor, step: int, out=None, tgt=None):
        seed = self.batch_seed(step)
        if self.mixer is not None:
            return self._make_mixed_batch(idx, seed, out, tgt)
        if self.device.type == "cuda":
            return augment_gpu(self.ds.images, self.ds.labels, idx, seed, self.train, self.pad, self.layout, out, tgt,
                               cutout=self.cutout)
        x, y = augment_cpu(self.ds.images, self.ds.labels, idx, seed, self.train, self.pad, self.layout,
                           cutout=self.cutout)
        if out is not None:
            out.copy_(x)
            tgt.copy_(y)
            return out, tgt
        return x, y

    def _make_mixed_batch(self, idx, seed, out, tgt):
        st = self.soft_targets
        B = idx.numel()
        if B > self.batch_size:
            raise ValueError("make_batch: more indices than batch_size (the soft-target buffers' size)")
        if self.device.type == "cuda":
            x, y, _, _ = augment_gpu(self.ds.images, self.ds.labels, idx, seed, True, self.pad, self.layout, out, tgt,
                                     mix=self.mixer, tgt_b=st.tgt_b, lam=st.lam, cutout=self.cutout)
            return x, y
        x, y, tb, lam = augment_cpu(self.ds.images, self.ds.labels, idx, seed, True, self.pad, self.layout,
                                    mix=self.mixer, cutout=self.cutout)
        st.tgt_b[:B].copy_(tb)
        st.lam[:B].copy_(lam)
        if out is not None:
            out.copy_(x)
            tgt.copy_(y)
            return out, tgt
        return x, y

    def cursor_batch(self, idx_all: torch.Tensor, nbatch: int, out, tgt, counter: torch.Tensor | None = None):
        """Batch k of ``idx_all`` (nbatch x batch_size indices) with augmentation seed ``batch_seed(k)``, k read
        on the device from ``counter`` (int32 [1]), written into the static ``out`` / ``tgt``.

        ``counter`` is the training step's own step counter (``SGD.step_counter()``: the LR-table kernel
        advances it once per step), so a captured step draws the next batch on every replay with no
        host work.  Without one, the loader keeps a private counter and advances it after the launch."""
        if self.device.type != "cuda":
            raise RuntimeError("cursor_batch needs the GPU-resident pipeline")
        own = counter is None
        if own:
            if getattr(self, "_cursor", None) is None:
                self._cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
            counter = self._cursor
        if counter.dtype != torch.int32 or not counter.is_cuda:
            raise ValueError("cursor_batch: counter must be an int32 device tensor")
        B = self.batch_size
        if idx_all.numel() < nbatch * B or idx_all.dtype != torch.int64 or not idx_all.is_cuda:
            raise ValueError("cursor_batch: idx_all must hold nbatch x batch_size int64 device indices")
        _, C, H, W = self.ds.images.shape
        if out.numel() < B * C * H * W or tgt.numel() < B:
            raise ValueError("cursor_batch: output buffers too small")
        lib = native.kernels()
        if self.mixer is not None:
            m, st = self.mixer, self.soft_targets
            rc = lib.ddpx_augment_mix_cursor(self.ds.images.data_ptr(), self.ds.labels.data_ptr(), idx_all.data_ptr(),
                                             nbatch, B, C, H, W, self.pad, self.batch_seed(0), self.cutout,
                                             LAYOUTS[self.layout], out.data_ptr(), tgt.data_ptr(), counter.data_ptr(),
                                             m.device_table(self.device).data_ptr(), m.cfg.modes, m.cfg.p_apply,
                                             m.cfg.p_switch, st.tgt_b.data_ptr(), st.lam.data_ptr(),
                                             native.stream_handle())
            native.check(rc, "ddpx_augment_mix_cursor")
            if own:
                counter.add_(1)
            return out, tgt
        rc = lib.ddpx_augment_cursor(self.ds.images.data_ptr(), self.ds.labels.data_ptr(), idx_all.data_ptr(), nbatch,
                                     B, C, H, W, self.pad, self.batch_seed(0), int(self.train), self.cutout,
                                     LAYOUTS[self.layout], out.data_ptr(), tgt.data_ptr(), counter.data_ptr(),
                                     native.stream_handle())
        native.check(rc, "ddpx_augment_cursor")
        if own:
            counter.add_(1)
        return out, tgt

    def valid_rows(self, step: int) -> int:
        """Rows of batch ``step`` that are samples of this rank's own: all of them, except where a sharded
        sampler's padding (the tail of the rank's index list) reaches into the last batches."""
        lo = step * self.batch_size
        rows = max(0, min(self.batch_size, len(self.sampler) - lo))
        return max(0, min(rows, self.sampler.num_valid() - lo))

    def __iter__(self):
        idx = self._epoch_indices()
        for step in range(len(self)):
            yield self.make_batch(idx[step * self.batch_size:(step + 1) * self.batch_size], step)

    @property
    def dataset(self):
        return self.ds
