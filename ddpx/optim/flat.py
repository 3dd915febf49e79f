"""What every optimizer over a flat parameter store shares: the binding, the device LR and one step driver.

All parameters are views of one flat fp32 buffer (``FlatParams``), so an update is a launch over a flat range.
:class:`FlatOptimizer` ties an optimizer to its store (state tensors laid out like the master, which a sharded
re-layout carries along), keeps the device learning-rate scalar / table and the clipping state, and owns
``step()``.  A step is a *schedule* (:meth:`FlatOptimizer._schedule`: which ranges, waited for how, on which
stream, followed by what) run by one driver (:meth:`FlatOptimizer._run`):

* for every pre-pass :class:`Stage` of the optimizer, in order: the partials unit by unit (the units are waited
  for in the first stage only; later ones find every bucket landed), the totals (under ZeRO-1 in two spans around
  ONE all-reduce of ``plan.sq``), the stage's finish;
* then the updates unit by unit (a unit is waited for here only when no stage ran), each followed by its gather;
* then, only with a ``ddpx.optim.WeightEMA`` attached (``self.ema``), its launches: the one post-update hook.

The schedules: ZeRO-1 (each rank updates its shard of every bucket as the reduce-scatter lands, on the current or
on the communicator stream), replicated overlap (each bucket as its all-reduce lands, on the compute or on a side
stream), and the local one (the whole store, or the runs of parameters not yet stepped).  A subclass supplies
``_update`` (the update rule over one range), its ``_stages`` and, if it counts steps on the device, ``_advance``.

Parameter groups.  An optimizer built with ``allow_groups=True`` takes several groups (without it more than one
group is refused, as it always was).  The groups together own exactly one store and may differ in ``lr``,
``weight_decay`` and, for LARS / LAMB, ``exclude_1d`` and ``adapt`` (:data:`PER_GROUP_KEYS`); any other key that
differs is a ``ValueError``.
They become one row ``{lr_mul, wd}`` per parameter in store order (:data:`Hyper`; ``ParamHyper`` on the device).  On
the CPU every parameter steps with its group's own current ``lr`` (bitwise torch's optimizers with the same groups).
On the GPU the device scalar / host value stays group 0's and a parameter's rate is that times its group's
multiplier ``base_i / base_0`` (``initial_lr`` if a scheduler set it, else ``lr``): one schedule for all groups, which
``sync_lr()`` checks.  While every row is the same (one group, equal groups) the optimizer launches exactly what it
launches without groups; otherwise ``_update`` takes the table-driven entry points over a chunk table built for the
schedule's ranges, and the fused backward is off (its kernels take one weight decay per launch).
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from functools import partial

import torch
from torch.optim import Optimizer

from ..runtime.flat_params import FlatParams, flat_of

# Device LR-schedule advance waiting for a kernel to carry it (device_lr_step): the classifier head's
# forward launch takes it (take_lr_advance), which saves the training step a separate 1-thread kernel;
# anything that reads lr before a head forward took it launches it on its own first (_flush_lr).
# The pending advance is a field of the parameter store the optimizer owns (``FlatParams.pending_lr``),
# so optimizers of different models in one process never hand their advances to each other.
# DDPX_LR_IN_HEAD=0 always launches the separate kernel.
_LR_IN_HEAD = os.environ.get("DDPX_LR_IN_HEAD", "1") != "0"


def take_lr_advance(flat):
    """(table, counter, lr) if the optimizer of ``flat`` has an LR advance pending (it is then the caller's
    launch that performs it), else None."""
    p = getattr(flat, "pending_lr", None)
    if p is None:
        return None
    flat.pending_lr = None
    return p


class Stage:
    """A pass over the whole gradient that must finish before any update (the global norm; LARS's per-parameter
    norms; LAMB's moments).  ``build(ranges)`` makes its plan (an object with ``reduce`` and ``sq``), cached until
    the ranges or ``key()`` change; ``partials(plan, k)`` launches the pass over range ``k``; ``finish(plan)`` runs
    once the totals are complete and leaves what the updates read."""

    def __init__(self, build, partials, finish, key=lambda: None):
        self.build, self.partials, self.finish, self.key = build, partials, finish, key
        self.plan = self._key = None

    def plan_for(self, ranges):
        key = ([(int(a), int(b)) for a, b in ranges], self.key())
        if self.plan is None or key != self._key:
            self.plan, self._key = self.build(key[0]), key
        return self.plan


# wait(): make the stream wait for the unit's gradient; pre: its indices into Schedule.ranges; update: the flat
# ranges to step; after(): what follows its updates (ZeRO-1: the bucket's all-gather)
Unit = namedtuple("Unit", "wait pre update after")
# ranges: what the stages' plans are built over; stream: a side stream for all of it (fork: behind an edge from the
# current stream; always joined back); src: the bucket source to tell optimizer_done; shards: the first ``shards``
# ranges are this rank's shards (their totals are all-reduced), None without ZeRO-1
Schedule = namedtuple("Schedule", "units ranges stream fork src shards")

# Parameter-group keys that may differ from group to group; every other key must be equal across the groups.
# ``adapt`` (LARS / LAMB; default True): False keeps the group's trust ratios at 1.
PER_GROUP_KEYS = ("params", "lr", "initial_lr", "weight_decay", "exclude_1d", "adapt")

# What the groups come to, parameter by parameter in store order.  group: the parameter's group index; lr_mul: its
# group's base learning rate over group 0's, rounded once to fp32 (base: the ``initial_lr`` a scheduler set, else
# ``lr``; a one-cycle schedule starts at lr = 0, so current values cannot define the ratio); wd: its weight decay;
# uniform: every row is the same and every lr_mul is 1 (one group, or equal ones): the optimizer launches exactly
# what it launches without groups; table: the device rows {lr_mul, wd} (``ParamHyper`` of
# csrc/include/ddpx_flat_optim.h; fp32 [P, 2]), None on the CPU and while uniform.
Hyper = namedtuple("Hyper", "group lr_mul wd uniform table")


def _f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


# parameter-group key -> (the optimizer whose state it marks, what a state without a family key gets told, whether
# the family takes exactly one group)
_STATE_KEYS = {"momentum": ("SGD", "no 'momentum' in its parameter group, keys {keys}", False),
               "betas": ("AdamW", "'betas' expected in its parameter groups, got keys {keys}", False),
               "trust_coef": ("LARS",), "exclude_1d": ("LAMB",)}


class FlatOptimizer(Optimizer):
    # parameter-group keys that identify this optimizer's state dict: {family key: True, variant key: present?}
    _state_keys = {}
    _advance = None        # _advance(group): the once-per-step counter advance, for an optimizer that has one
    _advance_stage = None  # the stage whose first launch it precedes (None: the first update launch)
    ema = None             # an attached ddpx.optim.WeightEMA: the step driver's one post-update hook

    def __init__(self, params, defaults, capturable=False, fused_backward=False, max_grad_norm=None, states=(),
                 allow_groups=False):
        """Tie the optimizer to the flat store that owns ``params``: the per-parameter state tensors ``states``
        (fp32 zeros laid out like the master), the device LR scalar, the clipping state and the DDP hooks."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        self.allow_groups = bool(allow_groups)
        super().__init__(list(params), defaults)
        if len(self.param_groups) != 1 and not self.allow_groups:
            # several groups are an explicit choice: they take the table-driven update and leave the fused backward
            raise ValueError(f"ddpx.optim.{type(self).__name__} supports a single parameter group unless built "
                             "with allow_groups=True (the groups may then differ in lr, weight_decay and, for LARS "
                             "and LAMB, exclude_1d and adapt)")
        params = self._all_params()
        flat = flat_of(params)
        if flat is None:
            raise ValueError("parameters are not flattened: wrap the model with ddpx.prepare_model() first")
        self.flat: FlatParams = flat
        self._hyper_cache = (None, None)
        self._update_plans = None  # the table-driven update's chunk plan (a Stage without passes), cached like one
        self._ranges = None        # the running schedule's ranges
        self._check_groups()
        for name in states:
            # registered with the store so a re-layout (sharded DDP) carries it along
            flat.state_tensors[name] = torch.zeros_like(flat.master)
        self.capturable = capturable
        # fused_backward: single-process training applies each parameter's update inside the kernel
        # that produces its gradient (no gradient round trip through HBM, no separate SGD pass).
        # max_grad_norm: clip the gradient to this global L2 norm before the update (clip_grad_norm_ + step in
        # one).  An attribute, not a param_group entry: state_dict() stays what torch's is.  Clipping
        # needs the whole gradient before any update, so it takes the materialised-gradient path.
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip = None       # device clip factor while a clipped step() runs its updates
        # [sum of squares, norm, clip factor] of the last step
        self._clip_res = (torch.zeros(3, dtype=torch.float32, device=flat.device)
                          if self.max_grad_norm is not None else None)
        self._stages = [self._clip_stage()] if self.max_grad_norm is not None else []
        # the fused kernels take one (momentum, weight_decay) per launch for several parameters: groups that
        # differ turn the fused backward off, as clipping does
        uniform = self._hyper().uniform  # (also refuses groups whose rates are no multiples of group 0's)
        self.fused_backward = bool(fused_backward and flat.master.is_cuda and self.max_grad_norm is None and uniform)
        need_dev_lr = capturable or self.fused_backward
        self._lr_dev = (torch.full((), float(defaults["lr"]), dtype=torch.float32, device=flat.device)
                        if need_dev_lr else None)
        if self.fused_backward:
            flat.fused_opt = self
        self._lr_table = None  # device-side LR schedule (attach_device_schedule)
        self._lr_counter = None
        self._advance_due = False
        self.bucket_source = None  # set by DDP when the optimizer overlaps the all-reduce or is sharded
        flat.optimizer = self
        if getattr(flat.sink, "sharded", False):
            flat.sink.attach_optimizer(self)
        self.step_count = 0

    def _clip_stage(self):
        """The global norm (``ddpx.ops.clip.GradNormPlan``) and the clip factor; every plan writes the optimizer's
        one result buffer, so ``grad_norm_dev`` is the same tensor for good."""
        from ..ops.clip import GradNormPlan

        def finish(plan):
            plan.coef(self.max_grad_norm)
            self._clip = plan.coef_dev
        return Stage(lambda ranges: GradNormPlan(self.flat, ranges, result=self._clip_res),
                     lambda plan, k: plan.partials(k), finish)

    # ------------------------------------------------------------------ parameter groups
    def _all_params(self):
        """Every group's parameters, in torch's state-dict order (the index running on across the groups)."""
        return [p for g in self.param_groups for p in g["params"]]

    def _check_groups(self):
        """The groups together own exactly one store and differ in ``PER_GROUP_KEYS`` only."""
        name = type(self).__name__
        if {id(p) for p in self._all_params()} != {id(p) for p in self.flat.params}:
            raise ValueError(f"{name} must own exactly the parameters of one FlatParams store")
        g0 = self.param_groups[0]
        for n, g in enumerate(self.param_groups[1:], 1):
            for key in sorted(set(g0) | set(g)):
                if key not in PER_GROUP_KEYS and (key not in g or key not in g0 or g[key] != g0[key]):
                    raise ValueError(f"ddpx.optim.{name}: parameter group {n} differs from group 0 in '{key}' "
                                     f"({g.get(key)!r} vs {g0.get(key)!r}); only lr, weight_decay, exclude_1d and "
                                     "adapt may differ between groups")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "flat"):  # (torch's constructor adds the initial groups through here, before the store)
            self._check_groups()
            self._hyper_cache = (None, None)
            if self.fused_backward and not self._hyper().uniform:
                self.disable_fused()

    def _hyper(self) -> Hyper:
        """The groups as per-parameter rows (:data:`Hyper`); rebuilt when a group's base lr, weight decay or
        membership or the store's layout changed (``add_param_group``, ``load_state_dict``, a ZeRO-1 relayout)."""
        f, groups = self.flat, self.param_groups
        base = [float(g.get("initial_lr", g["lr"])) for g in groups]
        key = (f.layout_version, tuple((b, float(g["weight_decay"]), len(g["params"])) for b, g in zip(base, groups)))
        if self._hyper_cache[0] == key:
            return self._hyper_cache[1]
        if any(b != base[0] for b in base) and base[0] == 0:
            raise ValueError(f"ddpx.optim.{type(self).__name__}: group 0's base learning rate is 0 while another "
                             "group's differs: the groups' rates are multiples of group 0's")
        mul = [1.0 if b == base[0] else _f32(b / base[0]) for b in base]
        group = [0] * len(f.params)
        for n, g in enumerate(groups):
            for p in g["params"]:
                group[f.index[id(p)]] = n
        lr_mul = [mul[n] for n in group]
        wd = [float(groups[n]["weight_decay"]) for n in group]
        uniform = all(m == 1.0 for m in lr_mul) and all(w == wd[0] for w in wd)
        table = None
        if f.master.is_cuda and not uniform:
            table = torch.tensor(list(zip(lr_mul, wd)), dtype=torch.float32).reshape(-1, 2).to(f.device)
        self._hyper_cache = (key, Hyper(group, lr_mul, wd, uniform, table))
        return self._hyper_cache[1]

    def _param_lrs(self, hyper: Hyper):
        """Each parameter's current learning rate, its group's own (store order): what the CPU path steps with."""
        return [float(self.param_groups[n]["lr"]) for n in hyper.group]

    def _plain(self):
        """LARS / LAMB: 1 for the parameters that keep a trust ratio of 1 (store order): their group has
        ``adapt=False``, or ``exclude_1d`` and the parameter has ``ndim <= 1``."""
        f = self.flat
        out = [0] * len(f.params)
        for g in self.param_groups:
            for p in g["params"]:
                out[f.index[id(p)]] = int((not g.get("adapt", True)) or (bool(g["exclude_1d"]) and p.dim() <= 1))
        return out

    def _update_plan(self):
        """The chunk table (every chunk with its parameter's index) the table-driven update of an optimizer
        without a stage of its own runs over: built for the schedule's ranges, cached like a stage's plan."""
        from ..ops.lars import PidChunkPlan
        if self._update_plans is None:
            self._update_plans = Stage(lambda ranges: PidChunkPlan(self.flat, ranges), None, None)
        return self._update_plans.plan_for(self._ranges if self._ranges is not None else [(0, self.flat.total)])

    def _check_lr_ratio(self):
        """Raise if the groups' current learning rates left the ratio of their base rates (the device holds group
        0's rate and one multiplier per group: per-group schedules are not implemented)."""
        groups = self.param_groups
        lr0 = float(groups[0]["lr"])
        if len(groups) < 2 or lr0 == 0:
            return
        base = [float(g.get("initial_lr", g["lr"])) for g in groups]
        for n, g in enumerate(groups[1:], 1):
            want = lr0 if base[n] == base[0] else lr0 * (base[n] / base[0])
            if not math.isclose(float(g["lr"]), want, rel_tol=1e-6, abs_tol=0.0):
                raise ValueError(f"ddpx.optim.{type(self).__name__}: group {n}'s learning rate {g['lr']!r} is not "
                                 f"{base[n]!r} / {base[0]!r} of group 0's {lr0!r}: the groups keep the ratio of "
                                 "their base rates (one schedule for all groups; per-group schedules are not "
                                 "implemented)")

    @property
    def lr_dev(self):
        """Device learning-rate scalar (None without one); current once any pending advance has run."""
        self._flush_lr()
        return self._lr_dev

    @property
    def grad_norm_dev(self):
        """Global L2 norm of the last step's gradient before clipping (0-d device fp32; None without
        ``max_grad_norm``).  Reading it on the host synchronises: do so where the loss is read."""
        return self._clip_res[1] if self._clip_res is not None else None

    @property
    def clip_coef_dev(self):
        """The factor the last step scaled its gradient by, min(1, max_norm / (norm + 1e-6)) (0-d device fp32)."""
        return self._clip_res[2] if self._clip_res is not None else None

    # ------------------------------------------------------------------ API
    def zero_grad(self, set_to_none: bool = True):  # noqa: D401 - torch signature
        self.flat.zero_grad()

    def fused_active(self) -> bool:
        return self.fused_backward

    def disable_fused(self):
        self.fused_backward = False
        if self.flat.fused_opt is self:
            self.flat.fused_opt = None

    def sync_lr(self):
        """Copy the host learning rate into the device scalar (outside graph capture).

        No-op while a device-side schedule is attached (the step kernel sequence advances it).  With several
        groups the scalar is group 0's; the others' rates are fixed multiples of it, which is checked here."""
        self._check_lr_ratio()
        self._hyper()  # (the table is built here, outside capture)
        if self._lr_dev is not None and self._lr_table is None:
            self._lr_dev.fill_(float(self.param_groups[0]["lr"]))

    def attach_device_schedule(self, scheduler, horizon: int | None = None):
        """Tabulate a LambdaLR-style schedule on the device (lr[k] = base_lr * lambda(k)).

        After this, :meth:`device_lr_step` — called at the start of every training step, inside the
        captured graph — sets ``lr_dev`` from the table and advances a device step counter, so graph
        replays need no host-to-device write.  The host scheduler keeps stepping for bookkeeping
        (state_dict, logging).  ``horizon``: table length (default: the one-cycle's end + 1).
        """
        if self._lr_dev is None or not self._lr_dev.is_cuda:
            return False
        lam = scheduler.lr_lambdas[0]
        base = scheduler.base_lrs[0]
        if horizon is None:
            spe, ne = getattr(lam, "steps_per_epoch", None), getattr(lam, "num_epochs", None)
            horizon = spe * ne + 1 if spe and ne else 100_000
        table = torch.tensor([base * lam(k) for k in range(horizon)], dtype=torch.float32)
        self._lr_table = table.to(self._lr_dev.device)
        self._lr_counter = torch.tensor([scheduler.last_epoch], dtype=torch.int32, device=self._lr_dev.device)
        return True

    def step_counter(self):
        """The device step counter the LR-table kernel advances once per ``device_lr_step`` (int32 [1]), or
        None without a device schedule; other per-step device work (the data cursor) may read it."""
        return getattr(self, "_lr_counter", None) if self._lr_table is not None else None

    def device_lr_step(self):
        if self._lr_table is None:
            return
        self._flush_lr()
        if _LR_IN_HEAD:
            self.flat.pending_lr = (self._lr_table, self._lr_counter, self._lr_dev)
            return
        self._launch_lr_advance()

    def _flush_lr(self):
        """Launch this optimizer's pending LR advance if no kernel took it (before anything reads lr)."""
        if getattr(self.flat, "pending_lr", None) is not None:
            self.flat.pending_lr = None
            self._launch_lr_advance()

    def _launch_lr_advance(self):
        from ..runtime import native
        native.check(native.kernels().ddpx_lr_advance(self._lr_table.data_ptr(), self._lr_table.numel(),
                                                      self._lr_counter.data_ptr(), self._lr_dev.data_ptr(),
                                                      native.stream_handle()), "ddpx_lr_advance")

    def _lr_arg(self):
        self._flush_lr()
        return self._lr_dev if self._lr_dev is not None else float(self.param_groups[0]["lr"])

    # ------------------------------------------------------------------ the step
    def _stepped(self, ranges):
        """``ranges`` (flat [start, end) pairs) minus the spans of parameters already stepped or skipped this
        iteration (``FlatParams.updated``): what the optimizer still has to update."""
        f = self.flat
        if not any(f.updated):
            return list(ranges)
        holes = [f.span(i, i) for i, u in enumerate(f.updated) if u]
        out = []
        for (s, e) in ranges:
            cur = s
            for (hs, he) in sorted(holes):
                if he <= cur or hs >= e:
                    continue
                if hs > cur:
                    out.append((cur, hs))
                cur = max(cur, he)
            if cur < e:
                out.append((cur, e))
        return out

    def _schedule(self) -> Schedule:
        f, src = self.flat, self.bucket_source
        if src is not None and getattr(src, "sharded", False):
            # ZeRO-1: each rank updates only its shard of every sharded bucket (gradients were reduce-scattered),
            # then the bucket's parameter copy is all-gathered in place.  With ``optimizer_stream`` all of it runs
            # on the communicator stream, in stream order behind each bucket's reduce-scatter: one compute -> comm
            # edge (end of backward: nothing still reads the weights) and one comm -> compute join at the end
            # instead of a join per bucket.
            side = src.optimizer_stream() if hasattr(src, "optimizer_stream") else None
            wait = src.wait_bucket if side is None else src.claim_bucket_on_comm_stream
            # the stages' ranges: the shards first, so that their totals are one span; the replicated buckets'
            # (the same on every rank) are added after the all-reduce
            ranges, pre = [], {}
            for b in sorted(range(len(src.bucket_ranges)), key=lambda b: src.bucket_modes[b] != 1):
                own = src.update_ranges(b)
                pre[b] = list(range(len(ranges), len(ranges) + len(own)))
                ranges += own
            shards = sum(len(pre[b]) for b in pre if src.bucket_modes[b] == 1)
            units = [Unit(partial(wait, b), pre[b], self._stepped(src.update_ranges(b)),
                          partial(src.gather_bucket, b)) for b in src.bucket_order()]
            return Schedule(units, ranges, side, True, src, shards)
        if not any(f.updated) and src is not None and src.overlap_active():
            # each bucket as its all-reduce lands (the pre-pass partials overlap the remaining collectives; every
            # rank holds the same reduced gradient, so the totals need no collective of their own).  With
            # ``update_side_stream`` on that stream, behind the bucket's all-reduce and its weights' release (no
            # wait for the end of backward) with one join into the compute stream; a pending LR advance (none
            # when the head kernel took it) is then launched there before the first update reads the LR.
            side = src.update_side_stream() if hasattr(src, "update_side_stream") else None
            units = []
            for (s, e) in src.bucket_ranges_in_completion_order():
                b = src.bucket_ranges.index((s, e))
                wait = partial(src.wait_range, s, e) if side is None else partial(src.side_wait_bucket, b, side)
                units.append(Unit(wait, [b], [(s, e)], None))
            return Schedule(units, src.bucket_ranges, side, False, src, None)
        # the whole store, or the runs of parameters a fused backward has not stepped already and that have a
        # gradient (one without was zeroed by fix_unwritten and adds 0 to a norm, as torch skips grad=None)
        runs, i, n = [], 0, len(f.params)
        while i < n:
            j = i
            while j < n and not f.updated[j]:
                j += 1
            if j > i:
                runs.append(f.span(i, j - 1))
            i = j + 1
        return Schedule([Unit(None, [0], runs, None)], [(0, f.total)], None, False, None, None)

    def _run(self, sch: Schedule, g):
        f = self.flat
        self._ranges = sch.ranges
        for n, st in enumerate(self._stages):
            plan = st.plan_for(sch.ranges)
            # a later stage finds every bucket landed; without shards it then goes in range order
            units = sch.units if n == 0 or sch.shards is not None else sorted(sch.units, key=lambda u: u.pre)
            for u in units:
                if n == 0 and u.wait is not None:
                    u.wait()
                for k in u.pre:
                    if st is self._advance_stage and self._advance_due and not all(f.updated):
                        # decided from the whole store, so every rank of a sharded run advances in the same steps
                        self._advance_due = False
                        self._advance(g)
                    st.partials(plan, k)
            if sch.shards is None:
                plan.reduce()
            else:  # SUM over the shard owners (on the current stream), then the replicated buckets' partials
                plan.reduce(span=(0, sch.shards))
                sch.src.comm.allreduce_(plan.sq, op="sum")
                if sch.shards < len(sch.ranges):
                    plan.reduce(accumulate=True, span=(sch.shards, len(sch.ranges)))
            st.finish(plan)
        for u in sch.units:
            if not self._stages and u.wait is not None:
                u.wait()
            for (start, end) in u.update:
                if self._advance_due and self._advance_stage is None:
                    self._advance_due = False
                    self._advance(g)
                if not self._advance_due:  # (still due: no launch of its stage, nothing has a gradient)
                    self._update(start, end, g, fp8=sch.shards is None)
            if u.after is not None:
                u.after()
        if self.ema is not None:
            # the weight average (ddpx.optim.WeightEMA): on this stream, before it is joined back.  ZeRO-1: the
            # ranges this rank updates (sch.ranges is every bucket's update_ranges); else the whole store
            self.ema.after_updates(sch.ranges if sch.shards is not None else [(0, f.total)])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        self._clip = None
        if not (self.flat.master.is_cuda and torch.cuda.is_current_stream_capturing()):
            # torch's optimizers skip a parameter whose .grad is None (no weight decay, no state update):
            # a parameter nobody produced a gradient for this step is marked as already stepped, so every
            # schedule leaves it alone (DDP's find_unused_parameters path marks the globally unused ones)
            for i in self.flat.fix_unwritten():
                self.flat.updated[i] = True
        # once per step, on the stream the step's launches go to, before the first launch that needs it
        self._advance_due = self._advance is not None
        sch = self._schedule()
        if sch.stream is None:
            self._run(sch, g)
        else:
            cur = torch.cuda.current_stream()
            if sch.fork:
                ev = torch.cuda.Event()
                ev.record(cur)
                sch.stream.wait_event(ev)
            with torch.cuda.stream(sch.stream):
                self._run(sch, g)
            done = torch.cuda.Event()
            done.record(sch.stream)
            cur.wait_event(done)
        if sch.src is not None:
            sch.src.optimizer_done()
        if sch.shards is not None:
            # the all-gathers refreshed master / bf16 copies of every shard, not the fp8 copy
            self.flat.fp8_mark(0, self.flat.total, False)
        self._clip = None
        if self._advance_due:
            # no parameter had a gradient: nothing was launched, and the step does not count (host or device)
            self._advance_due = False
        else:
            self.step_count += 1
        return loss

    # ------------------------------------------------------- (de)serialise
    def _check_state_kind(self, groups):
        """Raise unless ``groups`` (a state dict's parameter groups) carry this optimizer's ``_state_keys``."""
        (family, _), *variants = self._state_keys.items()
        name, detail, one_group = _STATE_KEYS[family]
        if (one_group and len(groups) != 1) or family not in groups[0]:
            detail = detail.format(keys=sorted(groups[0]) if groups else groups)
            raise ValueError(f"ddpx.optim.{name}.load_state_dict: not an {name} state ({detail}): was the "
                             "checkpoint written with another optimizer?")
        for key, want in variants:
            if (key in groups[0]) != want:
                kind = _STATE_KEYS[key][0]
                raise ValueError(f"ddpx.optim.{type(self).__name__}.load_state_dict: " +
                                 (f"not a {kind} state (no '{key}' in its parameter group)" if want else
                                  f"a {kind} state ('{key}' in its parameter group)") +
                                 ": was the checkpoint written with another optimizer?")
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                        for a, b in zip(groups, self.param_groups)):
            raise ValueError(f"ddpx.optim.{type(self).__name__}.load_state_dict: the state has "
                             f"{[len(a['params']) for a in groups]} parameters in its groups, the optimizer "
                             f"{[len(b['params']) for b in self.param_groups]}")

    def _load_groups(self, groups, skip=()):
        """Take every key but ``params`` (and ``skip``) of a state dict's parameter groups."""
        for mine, theirs in zip(self.param_groups, groups):
            for k, v in theirs.items():
                if k != "params" and k not in skip:
                    mine[k] = tuple(v) if k == "betas" else v
        self._check_groups()

    def _state_loaded(self):
        self._hyper_cache = (None, None)
        if self.fused_backward and not self._hyper().uniform:
            self.disable_fused()
        self._lr_table = None  # a resumed schedule position: re-attach the device schedule
        self.sync_lr()
