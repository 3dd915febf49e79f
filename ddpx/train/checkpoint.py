"""Checkpointing: the reference's format by default, full resumable state opt-in.

Default (``/root/reference/singlegpu.py:118-122``, ``multigpu.py:109-113``):
``torch.save(model_state_dict, "checkpoint.pt")`` — a plain ``OrderedDict``
with the module's own keys (no ``module.`` prefix: multigpu saves
``self.model.module.state_dict()``), each tensor its own storage on the model's
device, overwritten at every save.

Opt-in (absent in the reference): ``checkpoint_full.pt`` with
model, optimizer (momentum), scheduler, epoch, sampler epoch and RNG state,
written atomically (tmp file + ``os.replace``) so a crash never leaves a torn
file, and restored by :func:`load_full_checkpoint` for ``--resume``.

With a weight average (``ddpx.optim.WeightEMA``, ``--ema_decay``): ``checkpoint_ema.pt`` next to
``checkpoint.pt``, the same format with the averaged weights in place of the parameters (buffers are the
model's current ones), and the average's state under ``extra["ema"]`` of the full checkpoint.

With ``--save_best``: ``checkpoint_best.pt``, ``checkpoint.pt``'s format, rewritten whenever a validation's top-1
strictly improves (``Trainer._validate``).
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
from torch import nn

from ..models.resnet import tail_of

CKPT_PATH = "checkpoint.pt"
FULL_CKPT_PATH = "checkpoint_full.pt"
EMA_CKPT_PATH = "checkpoint_ema.pt"
BEST_CKPT_PATH = "checkpoint_best.pt"


def unwrap(model: nn.Module) -> nn.Module:
    return model.module if hasattr(model, "module") and isinstance(model.module, nn.Module) else model


def model_state_dict(model: nn.Module) -> "OrderedDict[str, torch.Tensor]":
    """state_dict of the unwrapped module with every tensor in its own storage."""
    sd = unwrap(model).state_dict()
    return OrderedDict((k, v.detach().clone()) for k, v in sd.items())


def _atomic_save(obj, path):
    tmp = f"{path}.tmp.{os.getpid()}"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def save_checkpoint(model: nn.Module, path: str = CKPT_PATH, atomic: bool = True):
    sd = model_state_dict(model)
    if atomic:
        _atomic_save(sd, path)
    else:
        torch.save(sd, path)
    return path


def save_ema_checkpoint(model: nn.Module, ema, path: str = EMA_CKPT_PATH):
    """``checkpoint.pt``'s format with the averaged weights (``ema``: a ``ddpx.optim.WeightEMA``; under ZeRO-1 after
    ``consolidate()``), written atomically.  Nothing is swapped: the model keeps training weights throughout."""
    sd = model_state_dict(model)
    for k, v in ema.params().items():
        sd[k] = v
    _atomic_save(sd, path)
    return path


def _tail_of(model):
    return tail_of(unwrap(model))


def tail_record(model) -> dict:
    """``extra`` entries of the full checkpoint for a model whose pooling tail is not the default one (ResNet-9 with
    ``tail="max"``): the tail has no parameters, so the state_dict cannot tell two tails apart.  The default tail
    records nothing (the file is then what it always was); :func:`load_full_checkpoint` reads a missing record as
    the default."""
    tail, scale = _tail_of(model)
    return {} if (tail, scale) == ("avg", 1.0) else {"tail": tail, "tail_scale": scale}


def save_full_checkpoint(path, model, optimizer, scheduler, epoch, extra=None):
    state = {
        "model": model_state_dict(model),
        "optimizer": optimizer.state_dict() if optimizer is not None else None,
        "scheduler": scheduler.state_dict() if scheduler is not None else None,
        "epoch": int(epoch),
        "torch_rng": torch.get_rng_state(),
        "extra": extra or {},
    }
    _atomic_save(state, path)
    return path


def load_full_checkpoint(path, model, optimizer=None, scheduler=None, map_location=None, ema=None):
    """Restore a full checkpoint written by :func:`save_full_checkpoint`; returns the next epoch.

    ``ema`` (a ``ddpx.optim.WeightEMA``): restored from ``extra["ema"]``; a file without one resets the average to
    the loaded weights, with a note."""
    state = torch.load(path, map_location=map_location, weights_only=True)
    m = unwrap(model)
    ex = state.get("extra") or {}
    saved_tail = (str(ex.get("tail", "avg")), float(ex.get("tail_scale", 1.0)))
    if saved_tail != _tail_of(m):
        raise ValueError(f"{path} was written with tail={saved_tail[0]!r} tail_scale={saved_tail[1]:g}, this run has "
                         f"tail={_tail_of(m)[0]!r} tail_scale={_tail_of(m)[1]:g}: resume with the same "
                         "--resnet_tail / --tail_scale")
    m.load_state_dict(state["model"])
    flat = getattr(next(m.parameters()), "_ddpx_flat", None)
    if flat is not None:
        flat.refresh_shadow()
    if optimizer is not None and state.get("optimizer") is not None:
        optimizer.load_state_dict(state["optimizer"])
    if scheduler is not None and state.get("scheduler") is not None:
        scheduler.load_state_dict(state["scheduler"])
    if ema is not None:
        saved = (state.get("extra") or {}).get("ema")
        if saved is not None:
            ema.load_state_dict(saved)
        else:
            ema.reset()
            print(f"note: {path} holds no EMA state: the weight average restarts from the loaded weights", flush=True)
    if state.get("torch_rng") is not None:
        torch.set_rng_state(state["torch_rng"].cpu())  # (map_location may have put it on the GPU)
    return int(state["epoch"]) + 1
