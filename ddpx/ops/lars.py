"""LARS over the flat store: per-parameter norms, the trust table and the trust-scaled flat SGD update.

LARS (You et al., 2017) scales each parameter tensor's SGD update by a trust ratio.  For every parameter ``i`` of
the store, with ``c`` the global clip factor (1 without clipping):

    wn_i = |w_i|      gn_i = c * |g_i|                                  (fp32 device scalars)
    adapt_i = not plain_i and wn_i > 0 and gn_i > 0                     (a NaN norm: False)
    t_i = trust_coef * wn_i / (gn_i + wd * wn_i + eps)  if adapt_i else 1
    d = t_i * (c * g + wd * w);  buf = mom * buf + d;  w -= lr * (d + mom * buf if nesterov else buf)

The passes (``csrc/kernels/lars.hip``), in the store-and-sum form of :mod:`ddpx.ops.clip`: two fp32 partials (w^2,
g^2) per chunk of at most :data:`CHUNK` elements of ONE parameter, per-parameter totals in fp64 in a fixed order, one
workgroup that forms the clip factor from the same totals (the gradient is read once) and writes the trust table,
and an update driven by the same chunk table in which every chunk carries its parameter's index.  No atomics and
no host read: reproducible bit for bit and graph-capturable.

CPU tensors take a torch path over the same tables; on the CPU that path defines the semantics.
"""
from __future__ import annotations

import bisect

import torch

from ..runtime import native
from .clip import CHUNK, ChunkPlan, build_chunks


def build_lars_chunks(offsets, numels, ranges, chunk: int = CHUNK):
    """:func:`ddpx.ops.clip.build_chunks` with the parameter index on every chunk: ``(start, len, pid)`` and the
    same ``spans``.  ``pid`` is the position in ``offsets`` (store order)."""
    chunks, spans = build_chunks(offsets, numels, ranges, chunk)
    starts = list(offsets)  # ascending: store order
    out = []
    for (s, n) in chunks:
        pid = bisect.bisect_right(starts, s) - 1
        assert starts[pid] <= s and s + n <= starts[pid] + numels[pid], (s, n, pid)
        out.append((s, n, pid))
    return out, spans


def _lr_args(lr):
    """(device pointer or None, host value) of a learning rate given as a float or a 0-d fp32 device tensor."""
    return (lr.data_ptr(), 0.0) if torch.is_tensor(lr) else (None, float(lr))


class PidChunkPlan(ChunkPlan):
    """A chunk table whose chunks carry their parameter's index, and the updates that need nothing more: the
    table-driven SGD and AdamW steps of optimizers with parameter groups (``hyper``: :data:`ddpx.optim.flat.Hyper`,
    whose device rows ``{lr_mul, wd}`` the kernels index with the chunk's ``pid``).  GPU only: on the CPU the
    optimizers step parameter by parameter with the scalar updates."""
    _cut = staticmethod(build_lars_chunks)

    def __init__(self, flat, ranges=None):
        super().__init__(flat, ranges)
        self._build()

    def _build(self):
        if super()._build():
            self._selected = {}
            return True
        return False

    def _hyper_table(self, hyper):
        t = hyper.table if hyper is not None else None
        if t is None or t.dtype != torch.float32 or t.numel() != 2 * len(self.flat.params) or \
                t.device != self.flat.master.device or not t.is_contiguous():
            raise ValueError("the hyper table must be a contiguous fp32 [P, 2] tensor on the store's device")
        return t

    def _sgd_chunks(self, what, start, end, lr, momentum, weight_decay, nesterov, first, grad_scale, clip,
                    momentum_buf, trust, hyper):
        """The checks and launches of :meth:`sgd_update` and :meth:`LarsPlan.update` (``what``: the caller's name
        in the messages): ``ddpx_sgd_flat_chunks`` over the chunks lying in ``[start, end)``, with the trust table,
        the hyper table or both.  CPU stores go to ``_update_cpu`` after the buffer checks."""
        f = self.flat
        runs = self._select(int(start), int(end))
        p, g, sh = f.master, f.grad, f.shadow
        n = p.numel()
        if g.numel() != n or (sh is not None and sh.numel() != n) or (momentum_buf is not None
                                                                      and momentum_buf.numel() != n):
            raise ValueError(f"{what}: buffers must have the store's numel")
        if momentum and momentum_buf is None:
            raise ValueError(f"{what}: a momentum needs the momentum buffer")
        if momentum_buf is not None and (momentum_buf.dtype != torch.float32 or momentum_buf.device != p.device):
            raise ValueError(f"{what}: the momentum buffer must be fp32 on the store's device")
        if not p.is_cuda:
            self._update_cpu(runs, lr, momentum, weight_decay if hyper is None else hyper.wd, nesterov, first,
                             grad_scale, clip, momentum_buf)
            return
        if clip is not None and (clip.dtype != torch.float32 or clip.device != p.device):
            raise ValueError(f"{what}: clip must be an fp32 scalar on the parameters' device")
        table = self._hyper_table(hyper) if hyper is not None else None
        lr_dev, lr_host = _lr_args(lr)
        lib = native.kernels()
        for (j, count) in runs:
            rc = lib.ddpx_sgd_flat_chunks(p.data_ptr(), native.ptr(momentum_buf), g.data_ptr(),
                                          int(g.dtype == torch.bfloat16), native.ptr(sh), self.table[j:].data_ptr(),
                                          count, native.ptr(trust), native.ptr(table), lr_dev, lr_host,
                                          float(momentum), float(weight_decay), float(grad_scale), native.ptr(clip),
                                          int(nesterov), int(first), native.stream_handle())
            native.check(rc, "ddpx_sgd_flat_chunks")

    def sgd_update(self, start: int, end: int, hyper, lr, momentum: float, nesterov: bool = False,
                   first: bool = False, grad_scale: float = 1.0, clip: torch.Tensor | None = None,
                   momentum_buf: torch.Tensor | None = None, trust: torch.Tensor | None = None):
        """``ddpx_sgd_flat_chunks`` with the hyper table over the chunks lying in ``[start, end)``: every parameter
        steps with its row's weight decay and ``lr * lr_mul`` (``trust``: optional fp32 ``[P]`` ratios, LARS).
        Padding between parameters is in no chunk and is not touched; the MX-FP8 copy is not written."""
        if not self.flat.master.is_cuda:
            raise ValueError("sgd update: the table-driven update is GPU only")
        self._hyper_table(hyper)
        self._sgd_chunks("sgd update", start, end, lr, momentum, 0.0, nesterov, first, grad_scale, clip,
                         momentum_buf, trust, hyper)

    def adamw_update(self, start: int, end: int, hyper, lr, exp_avg, exp_avg_sq, bc, beta1: float, beta2: float,
                     eps: float, grad_scale: float = 1.0, clip: torch.Tensor | None = None):
        """``ddpx_adamw_flat_hyper`` over the chunks lying in ``[start, end)``: ``adamw_flat_``'s step with every
        parameter's own weight decay and ``lr * lr_mul``."""
        f = self.flat
        runs = self._select(int(start), int(end))
        p, g, sh = f.master, f.grad, f.shadow
        n = p.numel()
        for t in (exp_avg, exp_avg_sq):
            if t.numel() != n or t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
                raise ValueError("adamw update: the states must be contiguous fp32 tensors of the store's numel")
        if g.numel() != n or (sh is not None and sh.numel() != n):
            raise ValueError("adamw update: buffers must have the store's numel")
        if bc is None or not bc.is_cuda or bc.dtype != torch.float32 or bc.numel() != 2:
            raise ValueError("adamw update: bc must be the fp32 [2] device tensor of adamw_advance_")
        if clip is not None and (clip.dtype != torch.float32 or clip.device != p.device):
            raise ValueError("adamw update: clip must be an fp32 scalar on the parameters' device")
        table = self._hyper_table(hyper)
        lr_dev, lr_host = _lr_args(lr)
        lib = native.kernels()
        for (j, count) in runs:
            rc = lib.ddpx_adamw_flat_hyper(p.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), g.data_ptr(),
                                           int(g.dtype == torch.bfloat16), native.ptr(sh),
                                           self.table[j:].data_ptr(), count, table.data_ptr(), lr_dev, lr_host,
                                           bc.data_ptr(), float(beta1), float(beta2), float(eps), float(grad_scale),
                                           native.ptr(clip), native.stream_handle())
            native.check(rc, "ddpx_adamw_flat_hyper")

    def _select(self, start, end):
        """Runs ``(first, count)`` of the chunk table lying in the flat range ``[start, end)``, which must cover
        exactly the parameters' elements inside it (its ends are parameter or range boundaries)."""
        self._build()
        hit = self._selected.get((start, end))
        if hit is not None:
            return hit
        idx = []
        for j, (s, n, _) in enumerate(self.chunks):
            if s >= start and s + n <= end:
                idx.append(j)
            elif s < end and s + n > start:
                raise ValueError(f"LarsPlan.update: [{start}, {end}) cuts the chunk [{s}, {s + n}): update ranges "
                                 "must end at parameter or plan-range boundaries")
        f = self.flat
        want = sum(max(0, min(o + n, end) - max(o, start)) for o, n in zip(f.offsets, f.numels))
        have = sum(self.chunks[j][1] for j in idx)
        if have != want:
            raise ValueError(f"LarsPlan.update: the plan's chunks cover {have} of the {want} parameter elements in "
                             f"[{start}, {end}) (the range is not inside the plan's ranges)")
        runs = []
        for j in idx:
            if runs and runs[-1][0] + runs[-1][1] == j:
                runs[-1][1] += 1
            else:
                runs.append([j, 1])
        self._selected[(start, end)] = runs
        return runs


class ParamNormPlan(PidChunkPlan):
    """Per-parameter totals over a chunk table whose chunks carry their parameter's index: the segment tables,
    :meth:`reduce`, the ``sq`` / ``trust`` / ``result`` buffers and the trust-table launch that
    :class:`LarsPlan` and :class:`ddpx.ops.lamb.LambPlan` share.  ``ranges``: flat ``[start, end)`` pairs this rank
    owns, non-overlapping; default the whole store.  Two fp32 partials per chunk: w^2 and the pass's own.

    ``sq`` (fp32 ``[2 P]``: w^2 totals then the other totals), ``trust`` (fp32 ``[P]``) and ``result`` (fp32
    ``[3]``: the global gradient sum of squares, norm and clip factor) may be caller-owned buffers.
    ``exclude_1d``: parameters with ``ndim <= 1`` (biases, BatchNorm affine) do not adapt; ``plain``: instead, a
    callable returning 0 / 1 per parameter in store order (1: does not adapt), asked again after a relayout.
    """
    _per_chunk = (2,)

    def __init__(self, flat, ranges=None, sq=None, trust=None, result=None, exclude_1d: bool = True, plain=None):
        ChunkPlan.__init__(self, flat, ranges)
        dev = flat.device
        P = self.P = len(flat.params)

        def own(t, n, what):
            if t is None:
                return None
            if t.dtype != torch.float32 or t.numel() != n or t.device != dev or not t.is_contiguous():
                raise ValueError(f"LarsPlan: {what} must be a contiguous fp32 [{n}] tensor on the store's device")
            return t.view(-1)
        self.sq = own(sq, 2 * P, "sq")
        if self.sq is None:
            self.sq = torch.zeros(2 * P, dtype=torch.float32, device=dev)
        self.trust_dev = own(trust, P, "trust")
        if self.trust_dev is None:
            self.trust_dev = torch.ones(P, dtype=torch.float32, device=dev)
        self._res = own(result, 3, "result")
        self.exclude_1d = bool(exclude_1d)
        self._plain_of = plain
        self._build()

    @property
    def sq_w(self):
        return self.sq[:self.P]

    @property
    def coef_dev(self):
        return self._res[2] if self._res is not None else None

    def _build(self):
        f = self.flat
        if len(f.params) != self.P:
            raise ValueError("LarsPlan: the store's parameter count changed")
        if super()._build():
            # 1: the parameter does not adapt (store order, so rebuilt with the layout)
            plain = ([int(bool(x)) for x in self._plain_of()] if self._plain_of is not None else
                     [int(self.exclude_1d and p.dim() <= 1) for p in f.params])
            self.plain = torch.tensor(plain, dtype=torch.int32).to(f.device)
            self._segments = {}

    def _segment_tables(self, k0, k1):
        """(order int32 [n], segments int32 [P, 2]) for the chunks of ranges ``k0 .. k1 - 1``: ``order`` lists
        their chunk indices parameter by parameter (table order inside one), ``segments[pid] = (first, count)``
        is the parameter's run in ``order`` (count 0: none of its elements are in these ranges)."""
        hit = self._segments.get((k0, k1))
        if hit is not None:
            return hit
        first = self.spans[k0][0] if k0 < len(self.spans) else self.n_chunks
        count = sum(c for _, c in self.spans[k0:k1])
        per = [[] for _ in range(self.P)]
        for j in range(first, first + count):
            per[self.chunks[j][2]].append(j)
        order, segs = [], []
        for idx in per:
            segs.append((len(order), len(idx)))
            order.extend(idx)
        dev = self.flat.device
        o = torch.tensor(order or [0], dtype=torch.int32).to(dev)
        s = torch.tensor(segs, dtype=torch.int32).reshape(-1, 2).to(dev)
        self._segments[(k0, k1)] = (o, s, order, segs)
        return self._segments[(k0, k1)]

    def reduce(self, accumulate: bool = False, span=None):
        """``sq`` (=|+=) the per-parameter sums of the partials, in a fixed order in fp64.  ``span = (k0, k1)``:
        only the partials of ranges ``k0 .. k1 - 1`` (default: all).  Without ``accumulate`` a parameter with no
        element in the span gets 0."""
        self._build()
        k0, k1 = (0, len(self.spans)) if span is None else span
        o, s, order, segs = self._segment_tables(k0, k1)
        if not self.flat.grad.is_cuda:
            P = self.P
            for pid, (first, count) in enumerate(segs):
                tot = self.partials_buf[order[first:first + count]].double().sum(0) if count else torch.zeros(
                    2, dtype=torch.float64)
                for h in (0, 1):
                    v = tot[h] + self.sq[h * P + pid].double() if accumulate else tot[h]
                    self.sq[h * P + pid] = v.float()
            return
        rc = native.kernels().ddpx_lars_segment_reduce(self.partials_buf.data_ptr(), o.data_ptr(), s.data_ptr(),
                                                       self.P, self.sq.data_ptr(), int(accumulate),
                                                       native.stream_handle())
        native.check(rc, "ddpx_lars_segment_reduce")

    def _trust_table(self, trust_coef: float, weight_decay: float, eps: float, max_norm: float | None = None,
                     hyper=None):
        """``trust_coef * wn / (gn + weight_decay * wn + eps)`` from ``sq`` where the parameter adapts, else 1;
        with ``max_norm`` also the global norm and clip factor (torch's ``clip_grad_norm_`` formula on the
        fixed-order fp64 sum of the second totals) into ``result``, the factor scaling every ``gn``.  ``hyper``
        (:data:`ddpx.optim.flat.Hyper`): every parameter's own weight decay instead of ``weight_decay``."""
        if max_norm is not None and self._res is None:
            raise ValueError("LarsPlan.trust: clipping needs the fp32 [3] result buffer")
        if not self.flat.grad.is_cuda:
            wn, gn = self.sq_w.sqrt(), self.sq[self.P:].sqrt()
            if max_norm is not None:
                total = self.sq[self.P:].double().sum().float()
                norm = total.sqrt()
                coef = torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)
                self._res[0], self._res[1], self._res[2] = total, norm, coef
                gn = coef * gn
            adapt = (self.plain == 0) & (wn > 0) & (gn > 0)
            wd = float(weight_decay) if hyper is None else torch.tensor(hyper.wd, dtype=torch.float32)
            t = (float(trust_coef) * wn) / ((gn + wd * wn) + float(eps))
            self.trust_dev.copy_(torch.where(adapt, t, torch.ones_like(t)))
            return
        table = self._hyper_table(hyper) if hyper is not None else None
        rc = native.kernels().ddpx_lars_trust(self.sq.data_ptr(), self.plain.data_ptr(), native.ptr(table), self.P,
                                              float(trust_coef), float(weight_decay), float(eps),
                                              float(max_norm) if max_norm is not None else 0.0,
                                              native.ptr(self._res), self.trust_dev.data_ptr(),
                                              native.stream_handle())
        native.check(rc, "ddpx_lars_trust")


class LarsPlan(ParamNormPlan):
    """:class:`ParamNormPlan` with LARS's passes.  Per step: :meth:`partials` for every range (in any order, as
    their gradients land), :meth:`reduce` (optionally in two spans around a SUM all-reduce of :attr:`sq`, as ZeRO-1
    needs), :meth:`trust`, then :meth:`update` for every range to step.  ``sq``: w^2 totals then g^2 totals;
    ``exclude_1d``: parameters with ``ndim <= 1`` keep plain SGD."""

    @property
    def sq_g(self):
        return self.sq[self.P:]

    def partials(self, k: int = 0):
        """Launch the sum-of-squares pass over range ``k``: (w^2, g^2) per chunk."""
        self._build()
        first, count = self.spans[k]
        if count == 0:
            return
        f = self.flat
        w, g = f.master, f.grad
        if not g.is_cuda:
            wd_, gd = w.detach(), g.detach()
            for j in range(first, first + count):
                s, n, _ = self.chunks[j]
                self.partials_buf[j, 0] = wd_[s:s + n].double().square().sum().float()
                self.partials_buf[j, 1] = gd[s:s + n].double().square().sum().float()
            return
        rc = native.kernels().ddpx_lars_sumsq(w.data_ptr(), g.data_ptr(), int(g.dtype == torch.bfloat16),
                                              self.table[first:].data_ptr(), count,
                                              self.partials_buf[first:].data_ptr(), native.stream_handle())
        native.check(rc, "ddpx_lars_sumsq")

    def trust(self, trust_coef: float, weight_decay: float, eps: float, max_norm: float | None = None, hyper=None):
        """The trust table from ``sq``; with ``max_norm`` also the global norm and clip factor into ``result``.
        ``hyper``: every parameter's own weight decay (parameter groups)."""
        self._trust_table(trust_coef, weight_decay, eps, max_norm, hyper)

    def compute(self, trust_coef: float, weight_decay: float, eps: float, max_norm: float | None = None):
        """All ranges, reduce, trust (single-process use)."""
        for k in range(len(self.ranges)):
            self.partials(k)
        self.reduce()
        self.trust(trust_coef, weight_decay, eps, max_norm)
        return self.trust_dev

    def update(self, start: int, end: int, lr, momentum: float, weight_decay: float, nesterov: bool = False,
               first: bool = False, grad_scale: float = 1.0, clip: torch.Tensor | None = None,
               momentum_buf: torch.Tensor | None = None, hyper=None):
        """The trust-scaled SGD step over the chunks lying in ``[start, end)`` (master, gradient and shadow are the
        store's; ``momentum_buf``: the store-sized momentum state, required with a momentum).  ``lr``: a float or
        a 0-d fp32 device tensor; ``clip``: a 0-d fp32 device factor on the gradient.  Padding between
        parameters is in no chunk and is not touched; the MX-FP8 copy is not written.  ``hyper`` (parameter
        groups): every parameter's own weight decay and, on the GPU, ``lr * lr_mul``; on the CPU ``lr`` is then the
        list of the parameters' own rates."""
        self._sgd_chunks("lars update", start, end, lr, momentum, weight_decay, nesterov, first, grad_scale, clip,
                         momentum_buf, self.trust_dev, hyper)

    def _update_cpu(self, runs, lr, momentum, weight_decay, nesterov, first, grad_scale, clip, momentum_buf):
        """``sgd_flat_``'s CPU sweep (torch.optim.SGD's op order) piece by piece, a piece being the consecutive
        chunks of one parameter, with ``d *= t`` after the weight decay; t == 1 changes no bit."""
        f = self.flat
        lrs = lr if isinstance(lr, (list, tuple)) else None  # per parameter (parameter groups)
        wds = weight_decay if isinstance(weight_decay, (list, tuple)) else None
        if lrs is None:
            lr_v = float(lr) if not torch.is_tensor(lr) else float(lr.item())
        if clip is not None:
            grad_scale = grad_scale * float(clip.item())
        pieces = []
        for (j, count) in runs:
            for (s, n, pid) in self.chunks[j:j + count]:
                if pieces and pieces[-1][2] == pid and pieces[-1][1] == s:
                    pieces[-1][1] = s + n
                else:
                    pieces.append([s, s + n, pid])
        trust = self.trust_dev.tolist()
        blk = 1 << 18
        tmp = torch.empty(blk, dtype=torch.float32)
        pf, gf = f.master.detach(), f.grad.detach()
        for (ps, pe, pid) in pieces:
            t = trust[pid]
            if lrs is not None:
                lr_v = float(lrs[pid])
            if wds is not None:
                weight_decay = float(wds[pid])
            for s in range(ps, pe, blk):
                e = min(pe, s + blk)
                p, g = pf[s:e], gf[s:e]
                d = tmp[:e - s]
                d.copy_(g)
                if grad_scale != 1.0:
                    d.mul_(grad_scale)
                if weight_decay:
                    d.add_(p, alpha=weight_decay)
                if t != 1.0:
                    d.mul_(t)
                if momentum:
                    b = momentum_buf[s:e]
                    if first:
                        b.copy_(d)
                    else:
                        b.mul_(momentum).add_(d)
                    if nesterov:
                        d.add_(b, alpha=momentum)
                    else:
                        d = b
                p.add_(d, alpha=-lr_v)
                if f.shadow is not None:
                    f.shadow[s:e].copy_(p)
