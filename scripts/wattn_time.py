#!/usr/bin/env python3
"""Times of the window self-attention blocks (docs/modes.md section 4w, docs/experiments/window_attention.md).

    python scripts/wattn_time.py kernels     forward and backward kernel alone at [16, 48, 48, 3 * 128], shift 0 and 4, and at one
                                             [1, 339, 510, 3 * 128] image: device-event median / best / worst of single launches, rotating
                                             through sets of tensors larger than the caches together, the bytes the algorithm needs,
                                             GB/s and the share of 6.29 TB/s
    python scripts/wattn_time.py steps       the captured pretrain step and the captured GAN step of the full-size Generator (batch 16,
                                             48 x 48 -> 192 x 192, 256 channels, 32 blocks) with --wattn_every 8 against off, alternating
    python scripts/wattn_time.py bytes       the byte counts alone (no device)

Method as in scripts/unet_d_time.py: device events around each launch, medians with best and worst, A and B alternating in one
process.  (The default benchmark against the parent commit is two checkouts and bench.py itself, alternating, parent first.)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.29e12
D = 128
SHAPES = [((16, 48, 48), 0), ((16, 48, 48), 4), ((1, 339, 510), 0), ((1, 339, 510), 4)]


def fwd_bytes(shape):
    """qkv read once, out written once"""
    n = shape[0] * shape[1] * shape[2]
    return 4 * n * (3 * D + D)


def bwd_bytes(shape):
    """qkv and dout read once, dqkv written once"""
    n = shape[0] * shape[1] * shape[2]
    return 4 * n * (3 * D + D + 3 * D)


def flops(shape, shift, backward=False):
    """issued by the MFMAs: 64 x 64 x 32 products, 2 per window and head forward, 7 backward (windows at the edge cost a whole one)"""
    wins = shape[0] * -(-(shape[1] + shift) // 8) * -(-(shape[2] + shift) // 8)
    return wins * (D // 32) * (7 if backward else 2) * 2 * 64 * 64 * 32


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


def _row(name, st, nbytes=None, nflops=None):
    med, lo, hi = (1e3 * v for v in st)
    tail = "" if nbytes is None else f"  {nbytes / 1e6:7.1f} MB  {nbytes / (med * 1e-6) / 1e9:6.0f} GB/s  {100 * nbytes / (med * 1e-6) / HBM:5.1f} % of 6.29 TB/s"
    if nflops is not None:
        tail += f"  {nflops / 1e9:5.2f} GFLOP  {nflops / (med * 1e-6) / 1e12:5.1f} TFLOP/s"
    print(f"{name:44s} {med:9.1f} us  (best {lo:9.1f}, worst {hi:9.1f}){tail}", flush=True)


def kernels():
    import torch
    from pesr_amd import ops
    for shape, shift in SHAPES:
        # eight sets of 76 MB (training shape) / six of 354 MB: more than the 256 MB of the last-level cache between two uses of a set
        sets = [(torch.randn(*shape, 3 * D, device="cuda"), torch.randn(*shape, D, device="cuda")) for _ in range(8 if shape[0] > 1 else 6)]
        _row(f"fwd {list(shape)} x {3 * D}, shift {shift}", _time(lambda q, g: ops.window_attention_fwd(q, shift), sets), fwd_bytes(shape),
             flops(shape, shift))
        _row(f"bwd {list(shape)} x {3 * D}, shift {shift}", _time(lambda q, g: ops.window_attention_bwd(q, g, shift), sets), bwd_bytes(shape),
             flops(shape, shift, True))
        del sets


def steps():
    import torch
    from model import VGG, Discriminator, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    B, S = 16, 192
    torch.manual_seed(0)
    V = VGG().cuda()
    lr, hr = torch.rand(B, 3, S // 4, S // 4, device="cuda") * 255, torch.rand(B, 3, S, S, device="cuda") * 255
    opt = {"num_channels": 256, "depth": 32, "res_scale": 0.1, "scale": 4, "patch_size": S // 4, "spectral_norm": False}
    for phase in ("pretrain", "train"):
        runs = {}
        for name, extra in (("off", {}), ("--wattn_every 8", {"wattn_every": 8, "wattn_dim": D})):
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
            print(f"{phase}, {name}: G has {sum(p.numel() for p in G.parameters()) / 1e6:.2f} M parameters", flush=True)
        for _ in range(3):
            for name, run in runs.items():
                _row(f"captured {phase} step, {name}", _time(lambda: run(lr, hr), [()], 10))
        del runs
        torch.cuda.empty_cache()


def bytes_():
    for shape, shift in SHAPES:
        print(f"{list(shape)} shift {shift}: forward {fwd_bytes(shape) / 1e6:.1f} MB, {flops(shape, shift) / 1e9:.2f} GFLOP; backward "
              f"{bwd_bytes(shape) / 1e6:.1f} MB, {flops(shape, shift, True) / 1e9:.2f} GFLOP")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "steps", "bytes"])
    {"kernels": kernels, "steps": steps, "bytes": bytes_}[ap.parse_args().what]()
