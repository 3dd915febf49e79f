"""Global gradient norm and clip factor over the flat gradient buffer (``clip_grad_norm_``).

All gradients of a model are one contiguous fp32 or bf16 buffer (``FlatParams.grad``); DDP buckets and ZeRO-1
shards are slices of it.  The norm is a streaming reduction over those slices in the store-and-sum form
(``csrc/kernels/grad_norm.hip``): one fp32 partial per chunk of at most :data:`CHUNK` elements of ONE parameter,
summed in a fixed order in fp64.  No atomics, so the result is bitwise reproducible; no value goes to the host,
so the whole path is graph-capturable.  The clip factor stays a device scalar that the flat SGD kernel folds
into its gradient scale (``sgd_flat_(..., clip=plan.coef_dev)``).

CPU tensors take an equivalent torch path over the same chunk table.
"""
from __future__ import annotations

import torch

from ..runtime import native

CHUNK = 32768  # elements per chunk (csrc/kernels/grad_norm.hip kChunk); a multiple of the store's alignment
ALIGN_ELEMS = 8  # chunk starts are multiples of this: 16 B for bf16 (and 32 B for fp32) gradients


def build_chunks(offsets, numels, ranges, chunk: int = CHUNK):
    """Cut the parameters ``(offsets[i], numels[i])`` intersected with the flat ``[start, end)`` ``ranges``
    into chunks ``(start, len)`` of at most ``chunk`` elements, each inside one parameter.

    Chunks start at multiples of ``chunk`` from the parameter's start or at a range boundary; the alignment
    padding between parameters is in no chunk.  Returns ``(chunks, spans)``: ``spans[k] = (first, count)`` are
    the chunks of range ``k`` (ranges in the given order, parameters in store order inside each).
    """
    chunks, spans = [], []
    for (rs, re_) in ranges:
        first = len(chunks)
        for o, n in zip(offsets, numels):
            lo, hi = max(o, rs), min(o + n, re_)
            cur = lo
            while cur < hi:
                nxt = min(hi, o + ((cur - o) // chunk + 1) * chunk)
                if cur % ALIGN_ELEMS:
                    raise ValueError(f"gradient chunk at flat element {cur} is not 16-B aligned "
                                     f"(range boundaries must be multiples of {ALIGN_ELEMS} elements)")
                chunks.append((cur, nxt - cur))
                cur = nxt
        spans.append((first, len(chunks) - first))
    return chunks, spans


class ChunkPlan:
    """The chunk table of ``flat`` over ``ranges``: flat ``[start, end)`` pairs (default: the whole store, whatever
    a later relayout makes its size); they must not overlap, or elements count twice.  The table is cached per
    ``(layout_version, ranges)`` and rebuilt only after a ``relayout``.  ``chunks`` are ``_cut``'s tuples
    ``(start, len[, pid])``, ``spans[k] = (first, count)`` the chunks of range ``k``, ``table`` the device rows
    and ``partials_buf`` one fp32 row of shape ``_per_chunk`` per chunk."""
    _cut = staticmethod(build_chunks)
    _per_chunk = ()

    def __init__(self, flat, ranges=None):
        self.flat = flat
        self._whole = ranges is None
        self.ranges = [(int(s), int(e)) for s, e in (ranges if ranges is not None else [(0, flat.total)])]
        self._key = None

    def _build(self) -> bool:
        """Rebuild the tables if the layout or the ranges changed; whether it did."""
        f = self.flat
        if self._whole:
            self.ranges = [(0, f.total)]
        key = (f.layout_version, tuple(self.ranges))
        if key == self._key:
            return False
        for (s, e) in self.ranges:
            if not 0 <= s <= e <= f.total:
                raise ValueError(f"range [{s}, {e}) outside the flat store [0, {f.total})")
        self.chunks, self.spans = self._cut(f.offsets, f.numels, self.ranges)
        self.n_chunks = len(self.chunks)
        # {int64 start; int32 len; int32 pid}: 16 bytes per entry (little endian: pid is the high half; 0 where the
        # chunks carry none)
        rows = [(c[0], c[1] + (sum(c[2:]) << 32)) for c in self.chunks]
        t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2) if rows else torch.zeros(0, 2, dtype=torch.int64)
        self.table = t.to(f.device)
        self.partials_buf = torch.zeros((max(1, self.n_chunks),) + self._per_chunk, dtype=torch.float32,
                                        device=f.device)
        self._key = key
        return True


class GradNormPlan(ChunkPlan):
    """Chunk table, partials buffer and result scalars for the gradient norm of ``flat`` over ``ranges``
    (:class:`ChunkPlan`).

    Per step: :meth:`partials` for every range (in any order, as their gradients land), :meth:`reduce`,
    optionally a SUM all-reduce of :attr:`sq` across shard owners, then :meth:`coef`.
    """

    def __init__(self, flat, ranges=None, result: torch.Tensor | None = None):
        super().__init__(flat, ranges)
        dev = flat.device
        # [sum of squares, norm, clip factor]; ``result``: a caller-owned fp32 [3] buffer to write instead
        if result is not None and (result.dtype != torch.float32 or result.numel() != 3 or result.device != dev):
            raise ValueError("GradNormPlan: result must be an fp32 [3] tensor on the store's device")
        self._res = result if result is not None else torch.zeros(3, dtype=torch.float32, device=dev)
        self.sq = self._res[0:1]
        self.norm_dev = self._res[1]
        self.coef_dev = self._res[2]
        self._build()

    # ------------------------------------------------------------------ passes
    def partials(self, k: int = 0):
        """Launch the sum-of-squares pass over range ``k``: one partial per chunk."""
        self._build()
        first, count = self.spans[k]
        if count == 0:
            return
        g = self.flat.grad
        if not g.is_cuda:
            gd = g.detach()
            for j in range(first, first + count):
                s, n = self.chunks[j]
                self.partials_buf[j] = gd[s:s + n].double().square().sum().float()
            return
        rc = native.kernels().ddpx_grad_sumsq(g.data_ptr(), int(g.dtype == torch.bfloat16),
                                              self.table[first:].data_ptr(), count,
                                              self.partials_buf[first:].data_ptr(), native.stream_handle())
        native.check(rc, "ddpx_grad_sumsq")

    def reduce(self, accumulate: bool = False, span=None):
        """``sq`` (=|+=) the sum of the partials, in a fixed order in fp64.  ``span = (k0, k1)``: only the
        partials of ranges ``k0 .. k1 - 1`` (default: all)."""
        self._build()
        if span is None:
            first, count = 0, self.n_chunks
        else:
            k0, k1 = span
            first = self.spans[k0][0] if k0 < len(self.spans) else self.n_chunks
            count = sum(c for _, c in self.spans[k0:k1])
        if not self.flat.grad.is_cuda:
            s = self.partials_buf[first:first + count].double().sum()
            if accumulate:
                s = s + self.sq[0].double()
            self.sq[0] = s.float()
            return
        rc = native.kernels().ddpx_grad_sumsq_reduce(self.partials_buf[first:].data_ptr() if count else None, count,
                                                     self.sq.data_ptr(), int(accumulate), native.stream_handle())
        native.check(rc, "ddpx_grad_sumsq_reduce")

    def coef(self, max_norm: float):
        """norm = sqrt(sq); clip factor = min(1, max_norm / (norm + 1e-6)) (torch's formula, NaN kept)."""
        if not self.flat.grad.is_cuda:
            norm = self.sq[0].sqrt()
            self._res[1] = norm
            self._res[2] = torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)
            return
        rc = native.kernels().ddpx_clip_coef(self.sq.data_ptr(), float(max_norm), self._res[1:].data_ptr(),
                                             native.stream_handle())
        native.check(rc, "ddpx_clip_coef")

    def compute(self, max_norm: float):
        """All ranges, reduce, factor (single-process use)."""
        for k in range(len(self.ranges)):
            self.partials(k)
        self.reduce()
        self.coef(max_norm)
        return self.norm_dev


def scale_dev_(x: torch.Tensor, scale: torch.Tensor):
    """In place ``x *= scale`` for a contiguous fp32 / bf16 buffer and a 0-d fp32 scalar on x's device."""
    if not x.is_cuda:
        return x.mul_(scale)
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise ValueError("scale_dev_: expected a contiguous fp32 or bf16 tensor")
    if scale.dtype != torch.float32 or scale.device != x.device:
        raise ValueError("scale_dev_: the scale must be an fp32 scalar on the tensor's device")
    rc = native.kernels().ddpx_scale_dev(x.data_ptr(), int(x.dtype == torch.bfloat16), x.numel(), scale.data_ptr(),
                                         native.stream_handle())
    native.check(rc, "ddpx_scale_dev")
    return x
