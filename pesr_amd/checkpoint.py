"""The training state file of train.py (--save_state_every / --resume): everything a run needs to go on as if it had never
stopped.  The reference keeps torch.save(G.state_dict()) alone ("no true resume"); this is an extension.

One torch.save dict (schema in INTEGRATION.md):
  format, flags {phase, scale, num_channels, num_blocks, spectral_norm, ema, attention, d_arch, wattn, wattn_norm}, epoch, best_psnr, G, D, optim_G, optim_D,
  scheduler_G, scheduler_D, dp {policy, transport}, world, rng [one entry per rank].
The file is written next to its final name and moved over it, so a run killed while writing leaves the previous file whole.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch

FORMAT = 1
STATE_NAME = "train_state.pt"
# the flags that decide the tensors' shapes and meaning: a state loads only into a run that agrees on all of them
SHAPE_FLAGS = ("phase", "scale", "num_channels", "num_blocks", "spectral_norm", "ema", "attention", "d_arch", "wattn", "wattn_norm")
# flags that joined later, with what a state written before them stands for (FORMAT stays 1: such a state still loads)
_LATER_FLAGS = {"attention": 0, "d_arch": "vgg", "wattn": 0, "wattn_norm": "none"}


def state_path(check_point: str, phase: str) -> str:
    return os.path.join(check_point, phase, STATE_NAME)


def resolve_resume(resume: str, check_point: str, phase: str):
    """--resume's value -> the file to load, or None for a fresh start.  "" is off; "auto" is the run's own state file if it is
    there (the same command line starts a run and restarts it); anything else is a path that has to exist."""
    if not resume:
        return None
    if resume == "auto":
        path = state_path(check_point, phase)
        return path if os.path.exists(path) else None
    if not os.path.exists(resume):
        raise SystemExit(f"train.py: --resume {resume}: no such file")
    return resume


def shape_flags(args) -> dict:
    return {"phase": args.phase, "scale": args.scale, "num_channels": args.num_channels, "num_blocks": args.num_blocks,
            "spectral_norm": bool(args.spectral_norm), "ema": args.ema_decay > 0,
            # the reduction of the Generator's channel attention, 0 = none (docs/modes.md section 4u)
            "attention": args.ca_reduction if getattr(args, "attention", "none") == "ca" else 0,
            # the Discriminator's kind (docs/modes.md section 4v); the pretrain phase has none and always says "vgg"
            "d_arch": getattr(args, "d_arch", "vgg") if args.phase != "pretrain" else "vgg",
            # the Generator's window-attention blocks (docs/modes.md section 4w): (--wattn_every, their width), 0 = none
            "wattn": wattn_flag(args),
            # the normalisation in front of those blocks' qkv (docs/modes.md section 4x): "ln" or "none"
            "wattn_norm": getattr(args, "wattn_norm", "none") or "none"}


def wattn_flag(args):
    every = getattr(args, "wattn_every", 0)
    return (every, getattr(args, "wattn_dim", 0) or args.num_channels // 2) if every > 0 else 0


def check_flags(state: dict, args, path: str = "") -> None:
    """SystemExit naming the first flag on which the state and this run disagree, with both values."""
    if state.get("format") != FORMAT:
        raise SystemExit(f"train.py: --resume {path}: state format {state.get('format')!r}, this version reads format {FORMAT}")
    mine = shape_flags(args)
    for k in SHAPE_FLAGS:
        theirs = state["flags"][k] if k not in _LATER_FLAGS else state["flags"].get(k, _LATER_FLAGS[k])
        if theirs != mine[k]:
            flag = {"ema": "--ema_decay > 0", "attention": "--attention / --ca_reduction (the reduction, 0 = none)",
                    "wattn": "--wattn_every / --wattn_dim (the period and the width, 0 = none)"}.get(k, "--" + k)
            raise SystemExit(f"train.py: --resume {path}: the state was saved with {flag} = {theirs!r}, this run has {mine[k]!r}")


def rng_snapshot(device=None, gpu_loader=None, shuffle=None) -> dict:
    """This rank's random streams: torch's CPU and device generators (the --GP interpolation weights are drawn on the device),
    Python's and numpy's, the GPU input pipeline's crop / augmentation stream (`gpu_loader`: an object with a random.Random `rng`)
    and the host loader's shuffle generator (`shuffle`: a torch.Generator)."""
    snap = {"torch": torch.random.get_rng_state(), "python": random.getstate(), "numpy": np.random.get_state()}
    if device is not None and torch.device(device).type == "cuda":
        snap["device"] = torch.cuda.get_rng_state(device)
    if gpu_loader is not None:
        snap["gpu_loader"] = gpu_loader.rng.getstate()
    if shuffle is not None:
        snap["shuffle"] = shuffle.get_state()
    return snap


def rng_restore(snap: dict, device=None, gpu_loader=None, shuffle=None) -> None:
    torch.random.set_rng_state(snap["torch"])
    random.setstate(snap["python"])
    np.random.set_state(snap["numpy"])
    if "device" in snap and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(snap["device"], device)
    if gpu_loader is not None and "gpu_loader" in snap:
        gpu_loader.rng.setstate(snap["gpu_loader"])
    if shuffle is not None and "shuffle" in snap:
        shuffle.set_state(snap["shuffle"])


def gather_rng(snap: dict, rank: int, world: int):
    """-> on rank 0 the list of every rank's snapshot (a collective: every rank calls it), None elsewhere."""
    if world == 1:
        return [snap]
    import torch.distributed as dist
    out = [None] * world if rank == 0 else None
    dist.gather_object(snap, out, dst=0)
    return out


def _cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def build_state(args, epoch, best_psnr, G, D, optim_G, optim_D, scheduler_G, scheduler_D, trainer, world, rng_list) -> dict:
    tr = trainer._transports()
    return {"format": FORMAT, "flags": shape_flags(args), "epoch": int(epoch), "best_psnr": float(best_psnr),
            "G": _cpu(G.state_dict()), "D": _cpu(D.state_dict()) if D is not None else None,
            "optim_G": _cpu(optim_G.state_dict()), "optim_D": _cpu(optim_D.state_dict()) if optim_D is not None else None,
            "scheduler_G": scheduler_G.state_dict(), "scheduler_D": scheduler_D.state_dict() if scheduler_D is not None else None,
            "dp": {"policy": trainer.dp_policy, "transport": type(tr[0]).__name__ if tr else None},
            "world": int(world), "rng": rng_list}


def atomic_save(state: dict, path: str) -> None:
    """torch.save to `path`.tmp, then os.replace: `path` is always either the previous file or the new one, never a part of one."""
    tmp = path + ".tmp"
    try:
        torch.save(state, tmp)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    os.replace(tmp, path)


def load_state(path: str) -> dict:
    # (the RNG entries are Python / numpy objects, not tensors: a full unpickle of a file this program wrote itself)
    return torch.load(path, map_location="cpu", weights_only=False)


def restore(state: dict, G, D, optim_G, optim_D, scheduler_G, scheduler_D) -> None:
    """Load the model, optimizer and scheduler entries IN PLACE: the parameters are views of the optimizers' flat buffers and
    stay that (Module.load_state_dict copies into them); FlatAdam.load_state_dict marks the packed weights stale."""
    G.load_state_dict(state["G"])
    optim_G.load_state_dict(state["optim_G"])
    scheduler_G.load_state_dict(state["scheduler_G"])
    if D is not None:
        D.load_state_dict(state["D"])
        optim_D.load_state_dict(state["optim_D"])
        scheduler_D.load_state_dict(state["scheduler_D"])
