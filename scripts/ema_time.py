#!/usr/bin/env python3
"""What the moving average of the Generator's weights costs (docs/modes.md section 4i), measured on the GPU:

  * the fused kernel (pesr_adam_ema_step, 36 B per parameter, one launch) against the plain Adam kernel followed by a separate
    torch lerp_ pass (28 + 12 B per parameter, two launches), and the plain Adam kernel alone, at the Generator's flat size;
    hot loops of --iters calls between two device events, the candidates alternated over --rounds rounds, median reported;
  * with --state_write: seconds per write of the full training state file (both full-size networks, both optimizers' moments and
    the average; about 1.65 GB at --patch_size 48) to a temporary directory.

    python scripts/ema_time.py [--n 43089956] [--iters 200] [--rounds 7] [--state_write [--patch_size 48]]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_times(n, iters, rounds, decay=0.999):
    from pesr_amd import ops
    dev = torch.device("cuda")
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
    m, v, e = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    args = (5e-5, 0.9, 0.999, 1e-8)

    def fused(k):
        ops.adam_ema_step(p, g, m, v, e, decay, *args, k)

    def separate(k):
        ops.adam_step(p, g, m, v, *args, k)
        e.lerp_(p, 1.0 - decay)

    def plain(k):
        ops.adam_step(p, g, m, v, *args, k)

    cands = {"adam_ema_fused": (fused, 36), "adam_then_lerp": (separate, 40), "adam_plain": (plain, 28)}
    for fn, _ in cands.values():                 # warm-up: code objects loaded, clocks up
        for k in range(1, 21):
            fn(k)
    torch.cuda.synchronize()
    us = {name: [] for name in cands}
    for _ in range(rounds):
        for name, (fn, _) in cands.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for k in range(1, iters + 1):
                fn(k)
            t1.record()
            torch.cuda.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    out = {}
    for name, (_, bytes_per) in cands.items():
        med = statistics.median(us[name])
        out[name] = {"us_median": round(med, 1), "us_min": round(min(us[name]), 1), "us_max": round(max(us[name]), 1),
                     "bytes_per_parameter": bytes_per, "TB_per_s": round(n * bytes_per / med / 1e6, 2)}
    return out


def state_write_time(patch_size, repeats=3):
    import importlib.util
    import torch.optim.lr_scheduler as lr_scheduler
    from model import Discriminator, Generator
    from pesr_amd import checkpoint
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("entry_train", os.path.join(root, "train.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    args = T.build_parser().parse_args(["--ema_decay", "0.999", "--patch_size", str(patch_size)])   # the full model
    opt = {"patch_size": args.patch_size, "num_channels": args.num_channels, "depth": args.num_blocks, "res_scale": args.res_scale,
           "spectral_norm": False, "scale": args.scale}
    G, D = Generator(opt).cuda(), Discriminator(opt).cuda()
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=5e-5, ema_decay=args.ema_decay)
    oD = FlatAdam(D.parameters(), lr=5e-5)
    oG.steps = oD.steps = 1                                               # (so the moments are part of the state)
    sG, sD = lr_scheduler.StepLR(oG, 120, 0.5), lr_scheduler.StepLR(oD, 120, 0.5)
    tr = Trainer(G, D, None, oG, oD)
    secs, size = [], 0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, checkpoint.STATE_NAME)
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = checkpoint.build_state(args, 1, 0.0, G, D, oG, oD, sG, sD, tr, 1, [checkpoint.rng_snapshot("cuda")])
            checkpoint.atomic_save(st, path)
            secs.append(time.perf_counter() - t0)
            size = os.path.getsize(path)
            del st
        t0 = time.perf_counter()
        checkpoint.load_state(path)
        load = time.perf_counter() - t0
    return {"seconds_per_write": [round(s, 2) for s in secs], "file_GB": round(size / 1e9, 3), "seconds_to_read": round(load, 2), "patch_size": patch_size,
            "parameters_G": oG.flat.numel, "parameters_D": oD.flat.numel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=43089956, help="floats in the flat buffer (default: the full Generator's)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--state_write", action="store_true")
    ap.add_argument("--patch_size", type=int, default=48,
                    help="with --state_write: the LR patch size, which sizes the Discriminator's classifier (48: bench.py's and the README's run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py measures on the GPU; none is visible")
    assert a.n % 4 == 0
    out = {"n": a.n, "iters": a.iters, "rounds": a.rounds, "kernels": kernel_times(a.n, a.iters, a.rounds)}
    if a.state_write:
        out["state_write"] = state_write_time(a.patch_size)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
