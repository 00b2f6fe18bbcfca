#!/usr/bin/env python3
"""Times of the channel LayerNorm in front of the window attention (docs/modes.md section 4x, docs/experiments/layernorm.md).

    python scripts/layernorm_time.py kernels     forward and backward kernel alone at [16, 48, 48, 256] and at one [1, 339, 510, 256]
                                                 image: device-event median / best / worst of single launches, rotating through sets of
                                                 tensors larger than the caches together, the bytes the algorithm needs, GB/s and the share
                                                 of 6.29 TB/s; pesr_ca_apply_fwd (two tensors read, one written, nothing else) on the same
                                                 tensors in the same process as the yardstick of what a streaming kernel reaches
    python scripts/layernorm_time.py steps       the captured pretrain step and the captured GAN step of the full-size Generator (batch 16,
                                                 48 x 48 -> 192 x 192, 256 channels, 32 blocks) with --wattn_every 8 --wattn_dim 128, without
                                                 and with --wattn_norm ln, alternating
    python scripts/layernorm_time.py bytes       the byte counts alone (no device)

Method as in scripts/wattn_time.py: device events around each launch, medians with best and worst, A and B alternating in one
process.  (The default benchmark against the parent commit is two checkouts and bench.py itself, alternating, parent first.)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.29e12
C = 256
SHAPES = [(16, 48, 48), (1, 339, 510)]


def _pixels(shape):
    return shape[0] * shape[1] * shape[2]


def fwd_bytes(shape):
    """x read once, y written once, 8 bytes of (mean, rstd) per pixel written"""
    return _pixels(shape) * (4 * 2 * C + 8)


def bwd_bytes(shape):
    """x and dy read once, dx written once, (mean, rstd) read; the partial rows of the channel sums written and read once"""
    from pesr_amd import ops
    return _pixels(shape) * (4 * 3 * C + 8) + 2 * ops.layernorm_partials(_pixels(shape), C) * 2 * C * 4


def ca_bytes(shape):
    """x and t read once, y written once"""
    return _pixels(shape) * 4 * 3 * C


def _stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def _time(fn, sets, reps=24):
    import torch
    for s in sets:
        fn(*s)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*sets[i % len(sets)]); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def _row(name, st, nbytes=None):
    med, lo, hi = (1e3 * v for v in st)
    tail = "" if nbytes is None else f"  {nbytes / 1e6:7.1f} MB  {nbytes / (med * 1e-6) / 1e9:6.0f} GB/s  {100 * nbytes / (med * 1e-6) / HBM:5.1f} % of 6.29 TB/s"
    print(f"{name:44s} {med:9.1f} us  (best {lo:9.1f}, worst {hi:9.1f}){tail}", flush=True)


def kernels():
    import torch
    from pesr_amd import ops
    gamma, beta = 1 + 0.5 * torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    gate = torch.rand(16, C, device="cuda")
    for shape in SHAPES:
        # (x, dy, stats): ten sets of 75 MB (training shape) / four of 354 MB - more than the 256 MB of the last-level cache between two
        # uses of a set, outputs included
        sets = []
        for _ in range(10 if shape[0] > 1 else 4):
            x, dy = 13 + 40 * torch.randn(*shape, C, device="cuda"), torch.randn(*shape, C, device="cuda")
            sets.append((x, dy, ops.layernorm_fwd(x, gamma, beta)[1]))
        for _ in range(2):      # (twice: the second round shows how far the figures repeat)
            _row(f"layernorm fwd {list(shape)} x {C}", _time(lambda x, dy, st: ops.layernorm_fwd(x, gamma, beta), sets), fwd_bytes(shape))
            _row(f"layernorm bwd {list(shape)} x {C}", _time(lambda x, dy, st: ops.layernorm_bwd(x, gamma, st, dy), sets), bwd_bytes(shape))
            _row(f"ca_apply_fwd  {list(shape)} x {C}", _time(lambda x, dy, st: ops.ca_apply_fwd(x, dy, gate[:shape[0]], 0.1), sets),
                 ca_bytes(shape))
        del sets
        torch.cuda.empty_cache()


def steps():
    import torch
    from model import VGG, Discriminator, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    B, S = 16, 192
    torch.manual_seed(0)
    V = VGG().cuda()
    lr, hr = torch.rand(B, 3, S // 4, S // 4, device="cuda") * 255, torch.rand(B, 3, S, S, device="cuda") * 255
    opt = {"num_channels": C, "depth": 32, "res_scale": 0.1, "scale": 4, "patch_size": S // 4, "spectral_norm": False, "wattn_every": 8,
           "wattn_dim": 128}
    for phase in ("pretrain", "train"):
        runs = {}
        for name, extra in (("--wattn_norm none", {}), ("--wattn_norm ln", {"wattn_norm": "ln"})):
            G = Generator(dict(opt, **extra)).cuda()
            oG = FlatAdam(G.parameters(), lr=5e-5)
            if phase == "pretrain":
                tr = Trainer(G, optim_G=oG)
            else:
                Dn = Discriminator(opt).cuda()
                tr = Trainer(G, Dn, V, oG, FlatAdam(Dn.parameters(), lr=5e-5))
            step = tr.gan_step if phase == "train" else tr.pretrain_step
            for _ in range(2):
                step(lr, hr)
            runs[name] = (tr.capture_gan_step if phase == "train" else tr.capture_pretrain_step)(lr, hr)
            print(f"{phase}, {name}: G has {sum(p.numel() for p in G.parameters()) / 1e6:.3f} M parameters", flush=True)
        for _ in range(3):
            for name, run in runs.items():
                _row(f"captured {phase} step, {name}", _time(lambda: run(lr, hr), [()], 10))
        del runs
        torch.cuda.empty_cache()


def bytes_():
    for shape in SHAPES:
        print(f"{list(shape)} x {C}: forward {fwd_bytes(shape) / 1e6:.1f} MB, backward {bwd_bytes(shape) / 1e6:.1f} MB, "
              f"ca_apply_fwd {ca_bytes(shape) / 1e6:.1f} MB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "steps", "bytes"])
    {"kernels": kernels, "steps": steps, "bytes": bytes_}[ap.parse_args().what]()
