"""The schedule of one ``step()`` of every flat optimizer, pinned as an ordered list of events (CPU, gloo).

For {SGD, SGD + clip, AdamW + clip, LARS, LARS + clip, LAMB, LAMB + clip} times {the whole store, one parameter
without a gradient, updates overlapped with the all-reduces, ZeRO-1}: what the step waits for, which pre-pass
launches run over which ranges, where the collectives, the totals and the finishing launches sit, which ranges are
updated (every update ends in ``FlatParams.fp8_mark``) and what follows each update.  The expected sequences are
literals, recorded before the optimizers were moved onto one step driver (``ddpx/optim/flat.py``): the file passes
unchanged on both sides of that change, and any later change of the schedule has to edit them on purpose.

Only names that are the plans' and the bucket source's public interface are wrapped.  The overlapped and ZeRO-1
cases run a real forward and backward through ``DistributedDataParallel`` at world size 1 (``reduce_single``); the
other two write the gradients by hand into a plain store.  The side-stream and communicator-stream schedules need a
GPU stream; the GPU suites check them bit for bit against the plain step.
"""
import warnings

import pytest
import torch
import torch.distributed as dist

from tests._dist_util import free_port, init_gloo

OPTS = {
    "sgd": ("SGD", dict(lr=0.1, momentum=0.9, weight_decay=5e-4)),
    "sgd_clip": ("SGD", dict(lr=0.1, momentum=0.9, weight_decay=5e-4, max_grad_norm=0.5)),
    "adamw_clip": ("AdamW", dict(lr=1e-3, max_grad_norm=0.5)),
    "lars": ("LARS", dict(lr=0.1, weight_decay=5e-4)),
    "lars_clip": ("LARS", dict(lr=0.1, weight_decay=5e-4, max_grad_norm=0.5)),
    "lamb": ("LAMB", dict(lr=1e-2)),
    "lamb_clip": ("LAMB", dict(lr=1e-2, max_grad_norm=0.5)),
}
MODES = ["whole", "nograd", "overlap", "zero1"]
NO_GRAD = 2  # a parameter in the middle of the store, so the "already stepped" branch updates two runs


@pytest.fixture(scope="module")
def gloo():
    init_gloo(0, 1, free_port())
    yield
    dist.destroy_process_group()


class _Recorder:
    def __init__(self, monkeypatch):
        self.events = []
        self.mp = monkeypatch
        self.depth = 0  # a plan method called by a plan method is not an event of the schedule

    def wrap(self, owner, name, fmt, plan=False):
        inner = getattr(owner, name)
        rec = self

        def wrapped(*a, **kw):
            if plan and rec.depth:
                return inner(*a, **kw)
            rec.events.append(fmt(*a, **kw))
            rec.depth += plan
            try:
                return inner(*a, **kw)
            finally:
                rec.depth -= plan
        self.mp.setattr(owner, name, wrapped)


def _plan_hooks(rec):
    from ddpx.ops.clip import GradNormPlan
    from ddpx.ops.lamb import LambPlan
    from ddpx.ops.lars import LarsPlan

    def tag(p):
        return "lamb" if isinstance(p, LambPlan) else "lars" if isinstance(p, LarsPlan) else "norm"

    def rng(p, k):
        return "%d=%d:%d" % ((k,) + tuple(p.ranges[k]))
    fmts = {
        "partials": lambda p, k=0: f"{tag(p)}.partials({rng(p, k)})",
        "moments": lambda p, k, *a, **kw: f"{tag(p)}.moments({rng(p, k)})",
        "reduce": lambda p, accumulate=False, span=None: "%s.reduce(%s%s)" % (
            tag(p), "all" if span is None else "%d:%d" % tuple(span), ",acc" if accumulate else ""),
        "coef": lambda p, *a: f"{tag(p)}.coef",
        "trust": lambda p, *a, **kw: f"{tag(p)}.trust",
        "update": lambda p, s, e, *a, **kw: f"{tag(p)}.update({s}:{e})",
        "apply": lambda p, s, e, *a, **kw: f"{tag(p)}.apply({s}:{e})",
    }
    seen = set()
    for cls in (GradNormPlan, LarsPlan, LambPlan):
        for name, fmt in fmts.items():
            # the class that defines the method, so that one shared by two plans is wrapped once
            owner = next((k for k in cls.__mro__ if name in k.__dict__), None)
            if owner is not None and (owner, name) not in seen:
                seen.add((owner, name))
                rec.wrap(owner, name, fmt, plan=True)


def _record(opt_key, mode, monkeypatch):
    import ddpx
    import ddpx.optim
    from ddpx.models import MLP
    from ddpx.parallel.comm import TorchComm
    from ddpx.parallel.ddp import DistributedDataParallel
    from ddpx.runtime.flat_params import FlatParams
    cls, hp = OPTS[opt_key]
    torch.manual_seed(0)
    model = MLP(hidden=64)
    ddpx.prepare_model(model, "cpu")
    opt = getattr(ddpx.optim, cls)(model.parameters(), **hp)
    flat = opt.flat
    assert max(flat.numels) == 196608  # fc0.weight: six chunks
    ddp = None
    if mode in ("overlap", "zero1"):
        ddp = DistributedDataParallel(model, comm=TorchComm(), bucket_cap_mb=0.001, first_bucket_mb=0.001,
                                      reduce_single=True, overlap_optimizer=mode == "overlap",
                                      shard_optimizer=mode == "zero1")
        ddp.attach_optimizer(opt)
        assert len(ddp.bucket_ranges) >= 3 and ddp.sharded == (mode == "zero1")
        g = torch.Generator().manual_seed(1)
        opt.zero_grad()
        loss, _ = ddp.forward_loss(torch.rand(8, 3072, generator=g), torch.randint(0, 10, (8,), generator=g))
        loss.backward()
    else:
        g = torch.Generator().manual_seed(1)
        opt.zero_grad()
        for i, p in enumerate(flat.params):
            if mode == "nograd" and i == NO_GRAD:
                continue
            p.main_grad.copy_(torch.randn(p.shape, generator=g) * 0.5)
            flat.grad_done(p)
    rec = _Recorder(monkeypatch)
    _plan_hooks(rec)
    rec.wrap(FlatParams, "fp8_mark", lambda f, s, e, w: f"mark({s}:{e},{bool(w)})")
    if ddp is not None:
        rec.wrap(ddp, "wait_bucket", lambda b: f"wait_bucket({b})")
        rec.wrap(ddp, "wait_range", lambda s, e: f"wait_range({s}:{e})")
        rec.wrap(ddp, "gather_bucket", lambda b: f"gather({b})")
        rec.wrap(ddp, "optimizer_done", lambda: "done")
        rec.wrap(ddp.comm, "allreduce_", lambda t, *a, **kw: f"allreduce({t.numel()})")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "parameters without gradient this step"
        opt.step()
    return rec.events


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt_key", list(OPTS))
def test_step_issues_the_recorded_schedule(opt_key, mode, gloo, monkeypatch):
    events = _record(opt_key, mode, monkeypatch)
    assert events == EXPECTED[f"{opt_key}-{mode}"].split(), "\n" + " ".join(events)


EXPECTED = {
    "sgd-whole": (
        "mark(0:201536,False)"
    ),
    "sgd-nograd": (
        "mark(0:704,False) mark(768:201536,False)"
    ),
    "sgd-overlap": (
        "wait_range(0:704) mark(0:704,False) wait_range(704:4864) mark(704:4864,False) wait_range(4864:201536) "
        "mark(4864:201536,False) done"
    ),
    "sgd-zero1": (
        "wait_bucket(0) mark(0:704,False) gather(0) wait_bucket(1) mark(704:4864,False) gather(1) wait_bucket(2) "
        "mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "sgd_clip-whole": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef mark(0:201536,False)"
    ),
    "sgd_clip-nograd": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef mark(0:704,False) mark(768:201536,False)"
    ),
    "sgd_clip-overlap": (
        "wait_range(0:704) norm.partials(0=0:704) wait_range(704:4864) norm.partials(1=704:4864) "
        "wait_range(4864:201536) norm.partials(2=4864:201536) norm.reduce(all) norm.coef mark(0:704,False) "
        "mark(704:4864,False) mark(4864:201536,False) done"
    ),
    "sgd_clip-zero1": (
        "wait_bucket(0) norm.partials(0=0:704) wait_bucket(1) norm.partials(1=704:4864) wait_bucket(2) "
        "norm.partials(2=4864:201536) norm.reduce(0:3) allreduce(1) norm.coef mark(0:704,False) gather(0) "
        "mark(704:4864,False) gather(1) mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "adamw_clip-whole": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef mark(0:201536,False)"
    ),
    "adamw_clip-nograd": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef mark(0:704,False) mark(768:201536,False)"
    ),
    "adamw_clip-overlap": (
        "wait_range(0:704) norm.partials(0=0:704) wait_range(704:4864) norm.partials(1=704:4864) "
        "wait_range(4864:201536) norm.partials(2=4864:201536) norm.reduce(all) norm.coef mark(0:704,False) "
        "mark(704:4864,False) mark(4864:201536,False) done"
    ),
    "adamw_clip-zero1": (
        "wait_bucket(0) norm.partials(0=0:704) wait_bucket(1) norm.partials(1=704:4864) wait_bucket(2) "
        "norm.partials(2=4864:201536) norm.reduce(0:3) allreduce(1) norm.coef mark(0:704,False) gather(0) "
        "mark(704:4864,False) gather(1) mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "lars-whole": (
        "lars.partials(0=0:201536) lars.reduce(all) lars.trust lars.update(0:201536) mark(0:201536,False)"
    ),
    "lars-nograd": (
        "lars.partials(0=0:201536) lars.reduce(all) lars.trust lars.update(0:704) mark(0:704,False) "
        "lars.update(768:201536) mark(768:201536,False)"
    ),
    "lars-overlap": (
        "wait_range(0:704) lars.partials(0=0:704) wait_range(704:4864) lars.partials(1=704:4864) "
        "wait_range(4864:201536) lars.partials(2=4864:201536) lars.reduce(all) lars.trust lars.update(0:704) "
        "mark(0:704,False) lars.update(704:4864) mark(704:4864,False) lars.update(4864:201536) "
        "mark(4864:201536,False) done"
    ),
    "lars-zero1": (
        "wait_bucket(0) lars.partials(0=0:704) wait_bucket(1) lars.partials(1=704:4864) wait_bucket(2) "
        "lars.partials(2=4864:201536) lars.reduce(0:3) allreduce(12) lars.trust lars.update(0:704) mark(0:704,False) "
        "gather(0) lars.update(704:4864) mark(704:4864,False) gather(1) lars.update(4864:201536) "
        "mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "lars_clip-whole": (
        "lars.partials(0=0:201536) lars.reduce(all) lars.trust lars.update(0:201536) mark(0:201536,False)"
    ),
    "lars_clip-nograd": (
        "lars.partials(0=0:201536) lars.reduce(all) lars.trust lars.update(0:704) mark(0:704,False) "
        "lars.update(768:201536) mark(768:201536,False)"
    ),
    "lars_clip-overlap": (
        "wait_range(0:704) lars.partials(0=0:704) wait_range(704:4864) lars.partials(1=704:4864) "
        "wait_range(4864:201536) lars.partials(2=4864:201536) lars.reduce(all) lars.trust lars.update(0:704) "
        "mark(0:704,False) lars.update(704:4864) mark(704:4864,False) lars.update(4864:201536) "
        "mark(4864:201536,False) done"
    ),
    "lars_clip-zero1": (
        "wait_bucket(0) lars.partials(0=0:704) wait_bucket(1) lars.partials(1=704:4864) wait_bucket(2) "
        "lars.partials(2=4864:201536) lars.reduce(0:3) allreduce(12) lars.trust lars.update(0:704) mark(0:704,False) "
        "gather(0) lars.update(704:4864) mark(704:4864,False) gather(1) lars.update(4864:201536) "
        "mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "lamb-whole": (
        "lamb.moments(0=0:201536) lamb.reduce(all) lamb.trust lamb.apply(0:201536) mark(0:201536,False)"
    ),
    "lamb-nograd": (
        "lamb.moments(0=0:201536) lamb.reduce(all) lamb.trust lamb.apply(0:704) mark(0:704,False) "
        "lamb.apply(768:201536) mark(768:201536,False)"
    ),
    "lamb-overlap": (
        "wait_range(0:704) lamb.moments(0=0:704) wait_range(704:4864) lamb.moments(1=704:4864) "
        "wait_range(4864:201536) lamb.moments(2=4864:201536) lamb.reduce(all) lamb.trust lamb.apply(0:704) "
        "mark(0:704,False) lamb.apply(704:4864) mark(704:4864,False) lamb.apply(4864:201536) mark(4864:201536,False) "
        "done"
    ),
    "lamb-zero1": (
        "wait_bucket(0) lamb.moments(0=0:704) wait_bucket(1) lamb.moments(1=704:4864) wait_bucket(2) "
        "lamb.moments(2=4864:201536) lamb.reduce(0:3) allreduce(12) lamb.trust lamb.apply(0:704) mark(0:704,False) "
        "gather(0) lamb.apply(704:4864) mark(704:4864,False) gather(1) lamb.apply(4864:201536) "
        "mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
    "lamb_clip-whole": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef lamb.moments(0=0:201536) lamb.reduce(all) lamb.trust "
        "lamb.apply(0:201536) mark(0:201536,False)"
    ),
    "lamb_clip-nograd": (
        "norm.partials(0=0:201536) norm.reduce(all) norm.coef lamb.moments(0=0:201536) lamb.reduce(all) lamb.trust "
        "lamb.apply(0:704) mark(0:704,False) lamb.apply(768:201536) mark(768:201536,False)"
    ),
    "lamb_clip-overlap": (
        "wait_range(0:704) norm.partials(0=0:704) wait_range(704:4864) norm.partials(1=704:4864) "
        "wait_range(4864:201536) norm.partials(2=4864:201536) norm.reduce(all) norm.coef lamb.moments(0=0:704) "
        "lamb.moments(1=704:4864) lamb.moments(2=4864:201536) lamb.reduce(all) lamb.trust lamb.apply(0:704) "
        "mark(0:704,False) lamb.apply(704:4864) mark(704:4864,False) lamb.apply(4864:201536) mark(4864:201536,False) "
        "done"
    ),
    "lamb_clip-zero1": (
        "wait_bucket(0) norm.partials(0=0:704) wait_bucket(1) norm.partials(1=704:4864) wait_bucket(2) "
        "norm.partials(2=4864:201536) norm.reduce(0:3) allreduce(1) norm.coef lamb.moments(0=0:704) "
        "lamb.moments(1=704:4864) lamb.moments(2=4864:201536) lamb.reduce(0:3) allreduce(12) lamb.trust "
        "lamb.apply(0:704) mark(0:704,False) gather(0) lamb.apply(704:4864) mark(704:4864,False) gather(1) "
        "lamb.apply(4864:201536) mark(4864:201536,False) gather(2) done mark(0:201536,False)"
    ),
}
