"""Orchestration shared by ``singlegpu.py`` and ``multigpu.py``.

Mirrors the reference's ``load_train_objs`` / ``prepare_dataloader`` /
``main`` / ``ddp_setup`` / ``__main__`` (``/root/reference/singlegpu.py:132-263``,
``multigpu.py:24-33,122-263``), keeping the positional CLI
(``TOTAL_EPOCHS SAVE_EVERY [--batch_size 512]``), the stdout lines and the
``checkpoint.pt`` format, and adding the SURVEY §5.6 flags.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import torch
import torch.distributed as dist

from ..data.datasets import DATASET_CLASSES, get_datasets
from ..data.loader import DeviceLoader
from ..data.sampler import DistributedIndexSampler
from ..models import build_model
from ..optim import decay_groups
from ..optim.schedule import one_cycle, resolve_steps_per_epoch
from ..optim.adamw import AdamW
from ..optim.ema import WeightEMA
from ..optim.lamb import LAMB
from ..optim.lars import LARS
from ..optim.sgd import SGD
from ..parallel.comm import HostStagedComm, RcclComm, TorchComm, set_rccl_protocol
from ..parallel.sync_bn import convert_sync_batchnorm
from ..parallel.ddp import DistributedDataParallel
from ..runtime.setup import prepare_model
from ..utils.metrics import MetricsWriter
from ..utils.size import MiB, get_model_size
from .checkpoint import FULL_CKPT_PATH, load_full_checkpoint
from .evaluate import evaluate, evaluate_metrics
from .trainer import Trainer

DEFAULT_DATA_ROOT = "data/cifar10"
REF_LR = 0.4
REF_MOMENTUM = 0.9
REF_WD = 5e-4
ADAMW_LR = 1e-3   # torch.optim.AdamW's defaults
ADAMW_WD = 1e-2
ADAMW_EPS = 1e-8
LAMB_EPS = 1e-6


def resolve_optimizer_defaults(args):
    """``--lr`` / ``--weight_decay`` left unset take the chosen optimizer's defaults: the reference's 0.4 / 5e-4
    for sgd and lars (LARS keeps the SGD recipe; its lr wants retuning), torch.optim.AdamW's 1e-3 / 1e-2 for adamw
    and lamb.  ``--eps`` left unset: 1e-6 for lamb, torch.optim.AdamW's 1e-8 otherwise."""
    adamw = getattr(args, "optimizer", "sgd") in ("adamw", "lamb")
    if getattr(args, "lr", None) is None:
        args.lr = ADAMW_LR if adamw else REF_LR
    if getattr(args, "weight_decay", None) is None:
        args.weight_decay = ADAMW_WD if adamw else REF_WD
    if getattr(args, "eps", None) is None:
        args.eps = LAMB_EPS if getattr(args, "optimizer", "sgd") == "lamb" else ADAMW_EPS
    return args


class _Parser(argparse.ArgumentParser):
    """Every parse ends with :func:`resolve_optimizer_defaults` (parse_args goes through parse_known_args)."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        own = DATASET_CLASSES.get(getattr(ns, "data", None))
        n = getattr(ns, "num_classes", None)
        if n is not None and n < 1:
            self.error("--num_classes must be positive")
        if n is not None and own is not None and n != own:
            self.error(f"--num_classes {n} contradicts --data {ns.data} ({own} classes)")
        if getattr(ns, "eval_every", 0) < 0 or getattr(ns, "topk", 0) < 0:
            self.error("--eval_every and --topk must not be negative")
        if getattr(ns, "save_best", False) and not getattr(ns, "eval_every", 0):
            self.error("--save_best needs --eval_every")
        tail, scale = getattr(ns, "resnet_tail", "avg"), getattr(ns, "tail_scale", 1.0)
        if getattr(ns, "model", "resnet9") != "resnet9" and (tail != "avg" or scale != 1.0):
            self.error("--resnet_tail / --tail_scale apply to --model resnet9 only")
        if tail == "avg" and scale != 1.0:
            self.error("--tail_scale needs --resnet_tail max")
        if getattr(ns, "cutout", 0) < 0:
            self.error("--cutout must not be negative")
        return resolve_optimizer_defaults(ns), rest


def build_parser(description: str) -> argparse.ArgumentParser:
    p = _Parser(description=description)
    p.add_argument("total_epochs", type=int, help="Total epochs to train the model")
    p.add_argument("save_every", type=int, help="How often to save a snapshot")
    p.add_argument("--batch_size", default=512, type=int, help="Input batch size on each device (default: 512)")
    p.add_argument("--model", default="vgg", choices=["vgg", "deepnn", "mlp", "mlp_wide", "resnet9"])
    p.add_argument("--resnet_tail", default="avg", choices=["avg", "max"],
                   help="resnet9: global average pool (default) or the published network's 4x4 max-pool in front of "
                        "the classifier")
    p.add_argument("--tail_scale", type=float, default=1.0, metavar="X",
                   help="resnet9 with --resnet_tail max: scale of the pooled features, applied inside the pooling "
                        "kernels (the published network: 0.125; default 1)")
    p.add_argument("--hidden", type=int, default=None, help="MLP hidden width (default 4096, wide 16384)")
    p.add_argument("--layers", type=int, default=3, help="MLP Linear layers (default 3)")
    p.add_argument("--data", default="auto", choices=["auto", "cifar10", "cifar100", "synthetic"])
    p.add_argument("--data_root", default=DEFAULT_DATA_ROOT,
                   help=f"dataset directory (default {DEFAULT_DATA_ROOT}; data/cifar100 with --data cifar100)")
    p.add_argument("--num_classes", type=int, default=None, metavar="N",
                   help="classes of the model and of synthetic data, at most 128 on the GPU (default: the "
                        "dataset's own, 10, or 100 for cifar100)")
    p.add_argument("--train_size", type=int, default=50000, help="synthetic train-set size")
    p.add_argument("--test_size", type=int, default=10000, help="synthetic test-set size")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "auto"],
                   help="compute precision: fp32 (default: the reference's recipe, /root/reference/singlegpu.py:134-141 "
                        "trains without autocast) or bf16 (MFMA bf16 with fp32 master weights; auto = bf16 on a GPU)")
    p.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"])
    p.add_argument("--kernels", default="auto", choices=["auto", "native", "torch"],
                   help="auto / native: the hand-written HIP kernels for every model and precision (measured faster "
                        "than MIOpen / hipBLASLt, profiles/r4_f32); torch: torch ops (MIOpen / hipBLASLt) under the "
                        "ddpx engine (flat store, fused SGD, native DDP)")
    p.add_argument("--bucket_cap_mb", type=float, default=None,
                   help="DDP bucket cap (default: calibrated on the node at start-up, see --bucket_plan)")
    p.add_argument("--first_bucket_mb", type=float, default=None)
    p.add_argument("--bucket_plan", default="calibrated", choices=["calibrated", "default"],
                   help="distributed: time a few training steps of every candidate gradient-communication plan "
                        "(bucket caps; replicated vs --shard_optimizer) on this node before training and use the "
                        "fastest (ddpx.parallel.calibrate); default = torch DDP's 25 / 1 MiB caps")
    p.add_argument("--steps_per_epoch", default="compat", help="'compat' (98/49 as the reference), 'auto' or N")
    p.add_argument("--seed", type=int, default=None, help="seed model init (reference: unseeded)")
    p.add_argument("--lr", type=float, default=None,
                   help="peak LR of the one-cycle schedule (default: the reference's 0.4 for sgd and lars, 1e-3 for adamw "
                        "and lamb)")
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "adamw", "lars", "lamb"],
                   help="sgd: the reference's SGD (momentum 0.9); adamw: torch.optim.AdamW semantics in one fused "
                        "flat kernel; lars: momentum SGD with layer-wise trust ratios (You et al. 2017) fused into the "
                        "flat update, for large global batches; lamb: Adam moments with layer-wise trust ratios (You et al. "
                        "2020), two flat passes, the Adam-family choice for large global batches (its lr is untuned "
                        "here).  adamw, lars and lamb take the unfused optimizer path at world size 1, as "
                        "--no_fused_optimizer")
    p.add_argument("--trust_coef", type=float, default=1e-3, help="lars: trust coefficient (default 1e-3)")
    p.add_argument("--lars_eps", type=float, default=1e-8, help="lars: epsilon of the trust ratio (default 1e-8)")
    p.add_argument("--betas", type=float, nargs=2, default=(0.9, 0.999), metavar=("B1", "B2"),
                   help="adamw, lamb: running-average coefficients (default 0.9 0.999)")
    p.add_argument("--eps", type=float, default=None,
                   help="adamw, lamb: denominator epsilon (default 1e-8 for adamw, 1e-6 for lamb)")
    p.add_argument("--weight_decay", type=float, default=None,
                   help="weight decay (default: the reference's 5e-4 for sgd and lars, 0.01 for adamw and lamb)")
    p.add_argument("--no_decay_1d", action="store_true",
                   help="no weight decay on biases and BatchNorm affine parameters (ndim <= 1): two parameter groups, "
                        "ddpx.optim.decay_groups (default off).  Single GPU: takes the unfused optimizer path, as "
                        "--no_fused_optimizer")
    p.add_argument("--graph", action="store_true",
                   help="capture the training step in a HIP graph (default on the GPU for the native kernels)")
    p.add_argument("--no_graph", action="store_true", help="eager training steps")
    p.add_argument("--grad_dtype", default="fp32", choices=["fp32", "bf16"], help="gradient buffer / all-reduce dtype")
    p.add_argument("--overlap_optimizer", action="store_true",
                   help="per-bucket SGD as all-reduces land (default when distributed)")
    p.add_argument("--no_overlap_optimizer", action="store_true", help="one SGD pass after all buckets landed")
    p.add_argument("--no_fused_optimizer", action="store_true",
                   help="single GPU: run SGD as its own pass instead of inside the backward kernels")
    p.add_argument("--clip_grad_norm", type=float, default=None, metavar="X",
                   help="clip the gradient to global L2 norm X before every update (torch's clip_grad_norm_; "
                        "default off).  Single GPU: takes the unfused optimizer path, as --no_fused_optimizer")
    p.add_argument("--ema_decay", type=float, default=None, metavar="D",
                   help="keep an exponential moving average of the weights with decay D (ddpx.optim.WeightEMA; default "
                        "off): one more fp32 buffer and one streaming pass per step; prints the averaged model's "
                        "accuracy after the fp32 one and writes checkpoint_ema.pt at every save")
    p.add_argument("--ema_warmup", action="store_true",
                   help="with --ema_decay: decay min(D, (1 + u) / (10 + u)) at update u")
    p.add_argument("--ema_every", type=int, default=1, metavar="K",
                   help="with --ema_decay: update the average on every K-th step with decay D^K (default 1)")
    p.add_argument("--label_smoothing", type=float, default=0.0, metavar="E",
                   help="train against (1 - E) * target + E / classes (F.cross_entropy's label_smoothing; default "
                        "0), formed inside the fused head's launch")
    p.add_argument("--mixup_alpha", type=float, default=0.0, metavar="A",
                   help="Mixup with lam ~ Beta(A, A), one draw per batch, partner = the batch reversed (timm's "
                        "batch mode; default off), mixed inside the batch's augment launch")
    p.add_argument("--cutmix_alpha", type=float, default=0.0, metavar="A",
                   help="CutMix with lam ~ Beta(A, A), one box per batch (default off)")
    p.add_argument("--mix_prob", type=float, default=1.0, metavar="P",
                   help="with --mixup_alpha / --cutmix_alpha: probability that a batch is mixed (default 1)")
    p.add_argument("--mix_switch_prob", type=float, default=0.5, metavar="P",
                   help="with both alphas: probability that a mixed batch uses CutMix (default 0.5)")
    p.add_argument("--cutout", type=int, default=0, metavar="S",
                   help="Cutout (DeVries & Taylor 2017): erase one SxS square per training sample to 0, its centre "
                        "drawn per sample, cut off at the border, inside the batch's augment launch (default 0: off)")
    p.add_argument("--tta_flip", action="store_true",
                   help="flip test-time augmentation: every evaluation scores the mean of the logits of each image "
                        "and of its mirror image (two forwards per batch; default off)")
    p.add_argument("--comm", default="rccl", choices=["rccl", "torch", "host"],
                   help="GPU collective backend (host: gloo-staged, lets several ranks share one GPU)")
    p.add_argument("--rccl_channels", default=None,
                   help="RCCL channel (CTA) bounds of the gradient communicator: N or MIN:MAX (default RCCL's)")
    p.add_argument("--rccl_proto", default=None, help="NCCL_PROTO for this job (Simple, LL, LL128)")
    p.add_argument("--shard_optimizer", action="store_true",
                   help="ZeRO-1: reduce-scatter grads, each rank updates its shard, all-gather params")
    p.add_argument("--chunk_mb", type=float, default=None,
                   help="split weights larger than this (MB of gradient) into row-chunk DDP buckets")
    p.add_argument("--side_optimizer", type=int, default=0,
                   help="DDP with optimizer overlap, replicated optimizer: each bucket's SGD update on a side stream "
                        "behind its all-reduce and its weights' last read in backward (0: on the compute stream)")
    p.add_argument("--comm_side_optimizer", action="store_true",
                   help="with --shard_optimizer on the RCCL path: shard updates on the communicator stream behind "
                        "each reduce-scatter (one join per step instead of one per bucket)")
    p.add_argument("--defer_gather", action="store_true",
                   help="with --shard_optimizer: all-gather updated shards at the start of the next forward, "
                        "overlapped with it (MLP native path)")
    p.add_argument("--sync_bn", action="store_true", help="SyncBatchNorm (reference: commented out)")
    p.add_argument("--resume", action="store_true", help=f"resume from {FULL_CKPT_PATH}")
    p.add_argument("--full_checkpoint", action="store_true", help=f"also write {FULL_CKPT_PATH}")
    p.add_argument("--metrics", default=None, help="JSON-lines metrics file")
    p.add_argument("--eval_batch", type=int, default=512)
    p.add_argument("--no_eval", action="store_true")
    p.add_argument("--eval_every", type=int, default=0, metavar="E",
                   help="validate on the test set after every E-th epoch: loss and top-1 (and --topk) printed and "
                        "logged to --metrics as event=eval, also for the averaged weights with --ema_decay (default 0: "
                        "only the final evaluation)")
    p.add_argument("--topk", type=int, default=0, metavar="K",
                   help="also report top-K accuracy in every validation and after the final accuracy lines (default "
                        "0: off)")
    p.add_argument("--shard_eval", action="store_true",
                   help="distributed: each rank evaluates its 1/N of the test set and the sums are added over the "
                        "ranks (default: every rank evaluates the whole set, as the reference does)")
    p.add_argument("--save_best", action="store_true",
                   help="with --eval_every: write checkpoint_best.pt whenever the validation top-1 strictly improves")
    p.add_argument("--nprocs", type=int, default=None, help="multigpu: processes to spawn (default: #GPUs)")
    p.add_argument("--fp8", action="store_true", help="MLP: MX-FP8 hidden-layer forward / weight-gradient GEMMs")
    p.add_argument("--profile", default=None, metavar="DIR",
                   help="re-run this command under rocprofv3 --kernel-trace --stats, output in DIR")
    p.add_argument("--debug", action="store_true",
                   help="serialised kernels (AMD_SERIALIZE_KERNEL=3, HIP_LAUNCH_BLOCKING=1) and DDP "
                        "bucket-order validation across ranks on every step")
    p.add_argument("--fault_step", type=int, default=None,
                   help="fault injection: rank --fault_rank raises at this global step")
    p.add_argument("--fault_rank", type=int, default=0)
    return p


def maybe_profile(args, argv=None) -> None:
    """``--profile DIR``: run this same command as a CHILD under rocprofv3 and exit with its code.

    Done before anything touches the GPU (rocprofv3's library initialises it in the child; this
    process never does), per SURVEY §5.1.  Output: DIR/<pid>/..._kernel_stats.csv etc.
    """
    if not getattr(args, "profile", None):
        return
    argv = list(sys.argv if argv is None else argv)
    rest, skip = [], False
    for a in argv[1:]:
        if skip:
            skip = False
            continue
        if a == "--profile":
            skip = True
            continue
        if a.startswith("--profile="):
            continue
        rest.append(a)
    out = os.path.abspath(args.profile)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(argv[0]), *rest]
    env = dict(os.environ, TMPDIR="/tmp")
    print("profiling:", " ".join(cmd), flush=True)
    rc = subprocess.run(cmd, env=env).returncode
    sys.exit(rc)


def apply_debug_env(args) -> None:
    """``--debug``: kernel serialisation for fault localisation (must precede GPU initialisation)."""
    if getattr(args, "debug", False):
        os.environ.setdefault("AMD_SERIALIZE_KERNEL", "3")
        os.environ.setdefault("HIP_LAUNCH_BLOCKING", "1")
        os.environ.setdefault("DDPX_DEBUG", "1")


def resolve_device(args, local_rank: int = 0) -> torch.device:
    if args.device == "cpu" or (args.device == "auto" and not torch.cuda.is_available()):
        return torch.device("cpu")
    return torch.device("cuda", local_rank)


def resolve_data(args):
    kind = args.data
    if kind == "auto":
        have = os.path.isdir(os.path.join(args.data_root, "cifar-10-batches-bin")) or os.path.isdir(
            os.path.join(args.data_root, "cifar-10-batches-py"))
        kind = "cifar10" if have else "synthetic"
    return kind


def resolve_data_root(args) -> str:
    """``--data_root``; left at its default, ``--data cifar100`` looks under data/cifar100."""
    if args.data == "cifar100" and args.data_root == DEFAULT_DATA_ROOT:
        return "data/cifar100"
    return args.data_root


def resolve_num_classes(args) -> int:
    """``--num_classes``, else the dataset's own: 100 for cifar100, 10 otherwise.  A real dataset's count cannot
    be overridden (``--data auto`` that found CIFAR-10 included)."""
    kind = resolve_data(args) if hasattr(args, "data") else "synthetic"  # (a namespace built by hand)
    own = DATASET_CLASSES.get(kind, 10)
    n = getattr(args, "num_classes", None)
    if n is None:
        return own
    if kind in DATASET_CLASSES and n != own:
        raise ValueError(f"--num_classes {n} contradicts the {kind} dataset ({own} classes)")
    return int(n)


def input_layout(model, device, dtype):
    if getattr(model, "input_layout", None):
        return model.input_layout(device)
    return "nchw_f32"


_CONFIG = None  # module-level run configuration the reference-signature helpers default to


def set_config(args) -> None:
    """Make ``args`` the configuration ``load_train_objs()`` / ``prepare_dataloader(ds, bs)`` use."""
    global _CONFIG
    _CONFIG = args


def current_config():
    """The active configuration: the one ``run()`` / ``set_config`` installed, else the reference's defaults
    (``TOTAL_EPOCHS=20 SAVE_EVERY=5``, VGG, lr 0.4, batch 512)."""
    global _CONFIG
    if _CONFIG is None:
        _CONFIG = build_parser("ddpx").parse_args(["20", "5"])
    return _CONFIG


def load_train_objs(args=None, device=None, distributed: bool = False, world_size: int = 1,
                    loader_len_hint: int | None = None, comm=None):
    """(train_set, model, optimizer, test_set, scheduler) — the reference's factory, ddpx engine underneath.

    Callable exactly as the reference does, ``load_train_objs()`` (``/root/reference/singlegpu.py:132``):
    every argument defaults from :func:`current_config` (device: the first GPU, else the CPU).

    ``--sync_bn`` (reference: the commented-out ``convert_sync_batchnorm`` at
    ``/root/reference/multigpu.py:127``): the native VGG merges BatchNorm statistics across ranks inside its
    own kernels' sequence (``model.sync_bn_comm``); the torch-op path swaps every BatchNorm2d for
    :class:`SyncBatchNorm2d` on ``comm`` before the flat parameter store is built.
    """
    if args is None:
        args = current_config()
    if device is None:
        device = resolve_device(args)
    if loader_len_hint is None:
        train_n = args.train_size if resolve_data(args) == "synthetic" else 50000
        loader_len_hint = _loader_len(train_n, args.batch_size, world_size)
    kind = resolve_data(args)
    train_set, test_set = get_datasets(kind, resolve_data_root(args), seed=0, train_size=args.train_size,
                                       test_size=args.test_size, num_classes=resolve_num_classes(args))
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model, optimizer = build_model_and_optimizer(args, device, distributed, comm)
    spe = resolve_steps_per_epoch(args.steps_per_epoch, loader_len_hint, distributed)
    scheduler = one_cycle(optimizer, spe)
    return train_set, model, optimizer, test_set, scheduler


def build_model_and_optimizer(args, device, distributed: bool = False, comm=None):
    """The model (native kernels where ``build_model`` puts them, SyncBatchNorm on request) in a flat parameter
    store, and its optimizer: ddpx SGD (the reference's lr 0.4 / momentum 0.9 / wd 5e-4) or, with
    ``--optimizer adamw`` / ``lars`` / ``lamb``, ddpx AdamW / LARS / LAMB."""
    model = build_model(args.model, hidden=args.hidden, layers=args.layers, dtype=args.dtype, device=device,
                        kernels=args.kernels, fp8=getattr(args, "fp8", False),
                        num_classes=resolve_num_classes(args), tail=getattr(args, "resnet_tail", "avg"),
                        tail_scale=getattr(args, "tail_scale", 1.0))
    if getattr(args, "sync_bn", False) and distributed:
        if getattr(model, "use_native", False) and device.type == "cuda":
            # native path, bf16 and fp32: the BN kernels merge statistics across ranks themselves
            # (ops/vgg_native.py, ops/f32.py bn_forward / bn_backward with comm)
            model.sync_bn_comm = comm
        else:
            model = convert_sync_batchnorm(model, comm)
    if args.graph and device.type == "cuda" and not getattr(model, "use_native", True):
        # torch-op models (--kernels torch: MIOpen / hipBLASLt ops) step eagerly: capturing torch's autograd with
        # AccumulateGrad nodes created by the eager warm-up steps is not supported (it crashed in bench.py)
        if getattr(args, "graph_explicit", True):
            print("note: --graph ignored for the torch-op model path", flush=True)
        args.graph = False
    prepare_model(model, device, grad_dtype=torch.bfloat16 if args.grad_dtype == "bf16" else torch.float32)
    resolve_optimizer_defaults(args)  # (a namespace built by hand)
    groups = bool(getattr(args, "no_decay_1d", False))
    params = decay_groups(model, args.weight_decay) if groups else model.parameters()
    if getattr(args, "optimizer", "sgd") == "adamw":
        optimizer = AdamW(params, lr=args.lr, betas=tuple(getattr(args, "betas", (0.9, 0.999))),
                          eps=args.eps, weight_decay=args.weight_decay,
                          capturable=bool(args.graph and device.type == "cuda"),
                          max_grad_norm=getattr(args, "clip_grad_norm", None), allow_groups=groups)
        return model, optimizer
    if getattr(args, "optimizer", "sgd") == "lamb":
        optimizer = LAMB(params, lr=args.lr, betas=tuple(getattr(args, "betas", (0.9, 0.999))),
                         eps=args.eps, weight_decay=args.weight_decay,
                         capturable=bool(args.graph and device.type == "cuda"),
                         max_grad_norm=getattr(args, "clip_grad_norm", None), allow_groups=groups)
        return model, optimizer
    if getattr(args, "optimizer", "sgd") == "lars":
        optimizer = LARS(params, lr=args.lr, momentum=REF_MOMENTUM, weight_decay=args.weight_decay,
                         trust_coef=getattr(args, "trust_coef", 1e-3), eps=getattr(args, "lars_eps", 1e-8),
                         capturable=bool(args.graph and device.type == "cuda"),
                         max_grad_norm=getattr(args, "clip_grad_norm", None), allow_groups=groups)
        return model, optimizer
    optimizer = SGD(params, lr=args.lr, momentum=REF_MOMENTUM, weight_decay=args.weight_decay,
                    capturable=bool(args.graph and device.type == "cuda"),
                    fused_backward=bool(not distributed and device.type == "cuda" and not args.no_fused_optimizer),
                    max_grad_norm=getattr(args, "clip_grad_norm", None), allow_groups=groups)
    return model, optimizer


def resolve_run_defaults(args, device, distributed: bool):
    """Defaults that depend on where the run happens (``run()``): HIP-graph steps on the GPU, and when
    distributed the per-bucket optimizer overlap and the node-calibrated bucket plan — the tuned path the
    benchmark measures, behind the reference's own entry points."""
    args.graph_explicit = bool(getattr(args, "graph", False))
    args.graph = bool(device.type == "cuda" and not getattr(args, "no_graph", False))
    if distributed:
        args.overlap_optimizer = bool(args.overlap_optimizer or not getattr(args, "no_overlap_optimizer", False))
    args.calibrate = bool(distributed and getattr(args, "bucket_plan", "default") == "calibrated"
                          and (args.bucket_cap_mb is None or args.first_bucket_mb is None))
    if not args.calibrate:
        if args.bucket_cap_mb is None:
            args.bucket_cap_mb = 25.0
        if args.first_bucket_mb is None:
            args.first_bucket_mb = 1.0


def make_ddp(args, model, optimizer, comm):
    net = DistributedDataParallel(model, comm=comm, bucket_cap_mb=args.bucket_cap_mb,
                                  first_bucket_mb=args.first_bucket_mb,
                                  overlap_optimizer=args.overlap_optimizer,
                                  shard_optimizer=args.shard_optimizer, chunk_mb=args.chunk_mb,
                                  defer_gather=args.defer_gather,
                                  comm_side_optimizer=args.comm_side_optimizer,
                                  side_stream_optimizer=bool(getattr(args, "side_optimizer", 0)))
    if args.overlap_optimizer or args.shard_optimizer:
        net.attach_optimizer(optimizer)
    return net


def _loss_of(net, model, x, y):
    if hasattr(model, "forward_loss"):
        loss, _ = net.forward_loss(x, y)
        return loss
    return torch.nn.functional.cross_entropy(net(x), y)


def calibrate_bucket_plan(args, device, comm, batch, world_size):
    """Start-up calibration of the DDP bucket plan (``ddpx.parallel.calibrate``), the same as ``bench.py``'s:
    every candidate (bucket caps; replicated, or ZeRO-1 when ``--shard_optimizer`` is given) is built for real
    on this node and a few training steps of it are timed (graph-captured when the run's steps are), and the
    fastest one's caps are written into ``args``.  Collective.  Returns {name, step_ms}."""
    import gc
    from ..parallel.calibrate import calibrate_by_step, candidate_plans
    from ..runtime.flat_params import flat_of
    from ..runtime.graphs import try_capture
    probe, _ = build_model_and_optimizer(args, device, True, comm)
    f = flat_of(probe)
    numels = list(f.numels)
    shapes = [tuple(p.shape) for p in f.params]
    shadow_only = [id(p) in f.shadow_only for p in f.params]
    del probe, f
    plans = [p for p in candidate_plans(numels, shadow_only, world_size, allow_shard=bool(args.shard_optimizer),
                                        shapes=None if args.chunk_mb else shapes)
             if p["shard"] == bool(args.shard_optimizer)]
    if not plans:
        args.bucket_cap_mb = 25.0 if args.bucket_cap_mb is None else args.bucket_cap_mb
        args.first_bucket_mb = 1.0 if args.first_bucket_mb is None else args.first_bucket_mb
        return {"chosen": "default", "step_ms": {}}
    x, y = batch
    cuda = device.type == "cuda"
    sync = torch.cuda.synchronize if cuda else (lambda: None)

    def make_trial(plan):
        a = argparse.Namespace(**vars(args))
        a.bucket_cap_mb = plan["bucket_cap_mb"] if args.bucket_cap_mb is None else args.bucket_cap_mb
        a.first_bucket_mb = plan["first_bucket_mb"] if args.first_bucket_mb is None else args.first_bucket_mb
        if not args.chunk_mb:
            a.chunk_mb = plan.get("chunk_mb")
        model, opt = build_model_and_optimizer(a, device, True, comm)
        net = make_ddp(a, model, opt, comm)
        one = torch.ones((), device=device)
        st = {"k": 0, "g": None}

        def body(xx, yy):
            opt.zero_grad()
            loss = _loss_of(net, model, xx, yy)
            loss.backward(one)
            opt.step()
            return loss

        def step():
            if a.graph and st["k"] >= 2 and st["g"] is None:
                st["g"], _ = try_capture(body, x, y, net, opt, comm=comm)
                if st["g"] is None:
                    a.graph = False
            if st["g"] is not None:
                st["g"]()
            else:
                body(x, y)
            st["k"] += 1

        def close():
            sync()
            st["g"] = None
            net.close()
            gc.collect()
            if cuda:
                torch.cuda.empty_cache()
        return step, close

    chosen, table = calibrate_by_step(plans, make_trial, sync=sync, warm=3, reps=5 if cuda else 2,
                                      rounds=3 if cuda else 1)
    if args.bucket_cap_mb is None:
        args.bucket_cap_mb = chosen["bucket_cap_mb"]
    if args.first_bucket_mb is None:
        args.first_bucket_mb = chosen["first_bucket_mb"]
    if not args.chunk_mb:
        args.chunk_mb = chosen.get("chunk_mb")
    return {"chosen": chosen["name"], "step_ms": table}


def mix_config(args):
    """The run's Mixup / CutMix configuration, or None when both are off (the loader is then the plain one)."""
    from ..data.mix import MixConfig
    cfg = MixConfig(getattr(args, "mixup_alpha", 0.0), getattr(args, "cutmix_alpha", 0.0),
                    getattr(args, "mix_prob", 1.0), getattr(args, "mix_switch_prob", 0.5))
    return cfg if cfg.enabled else None


def prepare_dataloader(dataset, batch_size: int, device=None, layout: str = "nchw_f32", rank: int = 0,
                       world_size: int = 1, seed: int = 0, mix=None, cutout: int = 0):
    """Shuffled training batches (``/root/reference/singlegpu.py:174``: ``DataLoader(dataset, batch_size,
    pin_memory=True, shuffle=True)``) produced on ``device`` by the GPU-resident loader.  Callable as
    ``prepare_dataloader(dataset, batch_size)``: NCHW fp32 batches on the configured device."""
    if device is None:
        device = resolve_device(current_config())
    sampler = DistributedIndexSampler(len(dataset), world_size, rank, shuffle=True, seed=seed)
    return DeviceLoader(dataset, batch_size, device, sampler=sampler, train=True, layout=layout, seed=seed + rank,
                        mix=mix, cutout=cutout)


def prepare_eval_loader(dataset, batch_size: int, device, layout: str = "nchw_f32", rank: int = 0,
                        world_size: int = 1, shard: bool = False):
    """Test batches in dataset order, unaugmented.  ``shard``: rank r of N takes samples r, r + N, ... (the sampler
    pads the tail by repeating the head; ``DeviceLoader.valid_rows`` keeps the padding out of the metrics); default:
    every rank walks the whole set (``/root/reference/multigpu.py:247``)."""
    sampler = None
    if shard and world_size > 1:
        sampler = DistributedIndexSampler(len(dataset), world_size, rank, shuffle=False)
    return DeviceLoader(dataset, batch_size, device, sampler=sampler, train=False, layout=layout)


def _loader_len(n, batch_size, world_size):
    per_rank = -(-n // world_size)
    return -(-per_rank // batch_size)


def run(args, rank: int = 0, world_size: int = 1, local_rank: int = 0, distributed: bool = False):
    set_config(args)
    device = resolve_device(args, local_rank)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    train_n = args.train_size if resolve_data(args) == "synthetic" else 50000
    comm = None
    if distributed:
        if device.type == "cuda" and args.comm == "rccl":
            set_rccl_protocol(getattr(args, "rccl_proto", None))
            comm = RcclComm(device, channels=getattr(args, "rccl_channels", None))
        elif device.type == "cuda" and args.comm == "host":
            comm = HostStagedComm()
        else:
            comm = TorchComm()
    resolve_run_defaults(args, device, distributed)
    dataset, model, optimizer, testdata, scheduler = load_train_objs(
        args, device, distributed, world_size, _loader_len(train_n, args.batch_size, world_size), comm)
    layout = input_layout(model, device, args.dtype)
    train_data = prepare_dataloader(dataset, args.batch_size, device, layout, rank, world_size, mix=mix_config(args),
                                    cutout=int(getattr(args, "cutout", 0) or 0))
    ema = None
    if getattr(args, "ema_decay", None) is not None:
        # before DDP: its re-layout carries the average and its initial broadcast makes it rank 0's on every rank
        ema = WeightEMA(optimizer, args.ema_decay, warmup=getattr(args, "ema_warmup", False),
                        every=getattr(args, "ema_every", 1))
    net = model
    if distributed:
        if args.calibrate:
            bs = min(args.batch_size, len(dataset))
            batch = train_data.make_batch(train_data._epoch_indices()[:bs], 0)
            cal = calibrate_bucket_plan(args, device, comm, batch, world_size)
            if rank == 0:
                print(f"bucket plan: calibrated {cal['chosen']} (first {args.first_bucket_mb:g} MB, cap "
                      f"{args.bucket_cap_mb:g} MB; training step ms per candidate: {cal['step_ms']})", flush=True)
        net = make_ddp(args, model, optimizer, comm)
    metrics = MetricsWriter(args.metrics, rank) if args.metrics else None
    topk = int(getattr(args, "topk", 0) or 0)
    if topk > resolve_num_classes(args):
        raise ValueError(f"--topk {topk} exceeds the {resolve_num_classes(args)} classes")
    shard_eval = bool(getattr(args, "shard_eval", False) and distributed)
    validation = {}
    test_data = None
    tta_flip = bool(getattr(args, "tta_flip", False))
    if getattr(args, "eval_every", 0) > 0 or shard_eval or topk or tta_flip:
        test_data = prepare_eval_loader(testdata, args.eval_batch, device, layout, rank, world_size, shard_eval)
    if getattr(args, "eval_every", 0) > 0:
        validation = dict(val_data=test_data, eval_every=args.eval_every, topk=topk,
                          save_best=bool(getattr(args, "save_best", False)), tta_flip=tta_flip)
    trainer = Trainer(net, train_data, optimizer, local_rank if device.type == "cuda" else rank, args.save_every,
                      scheduler, distributed=distributed, rank=rank, graph=args.graph, metrics=metrics,
                      full_checkpoint=args.full_checkpoint, ema=ema,
                      label_smoothing=getattr(args, "label_smoothing", 0.0), **validation)
    if args.fault_step is not None and rank == args.fault_rank:
        trainer.fault_step = args.fault_step
    if args.resume and os.path.exists(FULL_CKPT_PATH):
        trainer.start_epoch = load_full_checkpoint(FULL_CKPT_PATH, model, optimizer, scheduler,
                                                   map_location=device, ema=ema)
        if distributed:
            net._broadcast_state()

    start_time = time.time()
    trainer.train(args.total_epochs)
    if isinstance(net, DistributedDataParallel):
        net.consolidate()  # sharded optimizer: complete fp32 weights for eval / final state
    end_time = time.time()
    training_time = end_time - start_time
    print(f"Total training time: {training_time:.2f} seconds")

    fp32_model_size = get_model_size(model)
    print(f"fp32 model has size={fp32_model_size / MiB:.2f} MiB")
    if not args.no_eval and not (shard_eval or topk or tta_flip):
        if test_data is None:
            test_data = DeviceLoader(testdata, args.eval_batch, device, train=False, layout=layout)
        fp32_model_accuracy = evaluate(model, test_data)
        print(f"fp32 model has accuracy={fp32_model_accuracy:.2f}%")
        if ema is not None:
            with ema.applied():  # (collective under ZeRO-1; every rank evaluates, as above)
                ema_model_accuracy = evaluate(model, test_data)
            print(f"EMA model has accuracy={ema_model_accuracy:.2f}%")
    elif not args.no_eval:
        # --topk / --shard_eval / --tta_flip: the same lines from evaluate_metrics (its top-1 is evaluate()'s float),
        # the test set split over the ranks when sharded, and a top-K line after each
        group = dist.group.WORLD if shard_eval else None

        def final_lines(name):
            res = evaluate_metrics(model, test_data, topk, group, tta_flip=tta_flip)
            print(f"{name} model has accuracy={res.top1:.2f}%")
            if topk:
                print(f"{name} model has top-{topk} accuracy={res.topk:.2f}%")

        final_lines("fp32")
        if ema is not None:
            with ema.applied():
                final_lines("EMA")
    if metrics is not None:
        metrics.log(event="done", training_time=training_time)
        metrics.close()
    if comm is not None:
        if device.type == "cuda":
            torch.cuda.synchronize()
        if isinstance(net, DistributedDataParallel):
            net.close()
        comm.close()
    return model


# ------------------------------------------------------------------ multi
def ddp_setup(rank: int, world_size: int, device_type: str, comm: str = "rccl"):
    """Rendezvous (reference: multigpu.py:24-33).  Env MASTER_ADDR/PORT win over the defaults.

    With the native RCCL communicator the c10d group only bootstraps it (TCPStore) and carries
    CPU-side metadata, so it is gloo; ``--comm torch`` uses stock ProcessGroupNCCL (RCCL) instead.
    """
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "12355")
    if device_type == "cuda":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
        backend = "gloo" if comm == "rccl" else "cpu:gloo,cuda:nccl"
    else:
        backend = "gloo"
    dist.init_process_group(backend=backend, rank=rank, world_size=world_size)


def main_multi(rank: int, world_size: int, args):
    """Per-process entry (mp.spawn target or torchrun worker)."""
    device_type = resolve_device(args).type
    ddp_setup(rank, world_size, device_type, args.comm)
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    try:
        run(args, rank=rank, world_size=world_size, local_rank=local_rank, distributed=True)
    finally:
        dist.destroy_process_group()
