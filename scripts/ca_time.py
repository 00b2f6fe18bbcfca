#!/usr/bin/env python3
"""Times of the channel attention (docs/modes.md section 4u, docs/experiments/channel_attention.md), device events throughout.

    python scripts/ca_time.py kernels [--out FILE]      every kernel at the training shape [16, 48, 48, 256], reduction 16: time, the
                                                        bytes the algorithm needs (from the shapes), GB/s and the share of 6.29 TB/s;
                                                        on one set of tensors (a 37.7 MB tensor stays in the 256 MiB last-level cache)
                                                        and rotating through eight sets (906 MB: every read comes from HBM)
    python scripts/ca_time.py steps [--out FILE]        captured pretrain and GAN step of the full-size networks (batch 16, 48 -> 192,
                                                        256 x 32), attention off / on, every variant twice, alternating; the floor of
                                                        the added kernels computed from bytes
    python scripts/ca_time.py once                      every kernel at the training shape once cold (after a 512 MB fill) and once
                                                        warm (for a counters-only profiler run: FETCH_SIZE per dispatch)
    python scripts/ca_time.py bytes                     the byte counts alone (needs no device)

One JSON document on stdout (and in FILE)."""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _loss_time import HBM_TBS, time_events  # noqa: E402
import torch  # noqa: E402

SHAPE, REDUCTION, RES_SCALE, BLOCKS = (16, 48, 48, 256), 16, 0.1, 32


def tensor_bytes(shape=SHAPE):
    n = 4
    for d in shape:
        n *= d
    return n


def algorithm_bytes(shape=SHAPE, reduction=REDUCTION):
    """The bytes each kernel's algorithm needs, from the shapes: activations read and written once, the small tensors too."""
    N, H, W, C = shape
    R = C // reduction
    T, v, h, w = tensor_bytes(shape), 4 * N * C, 4 * N * R, 4 * (2 * C * R + C + R)
    return {"pool": T + v, "ds": 2 * T + v, "apply_fwd": 3 * T + v, "apply_bwd": 2 * T + 2 * v,
            "gate_fwd": v + w + h + v, "gate_bwd": 3 * v + h + w + v + w}


def block_floor_bytes(shape=SHAPE):
    """Per block: forward reads t twice and x once and writes y; backward reads gy twice and t once and writes gt."""
    return {"forward": 4 * tensor_bytes(shape), "backward": 4 * tensor_bytes(shape)}


def _sets(count, dev):
    from pesr_amd import ops
    N, H, W, C = SHAPE
    R = C // REDUCTION
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    w1, b1, w2, b2 = rnd(R, C) / 16, rnd(R) / 10, rnd(C, R) / 4, rnd(C) / 10
    out = []
    for _ in range(count):
        x, t, gy = rnd(*SHAPE), rnd(*SHAPE) / 2, rnd(*SHAPE) / 100
        m = ops.ca_pool(t)
        h, s = ops.ca_gate_fwd(m, w1, b1, w2, b2)
        ds = ops.ca_ds(gy, t, RES_SCALE)
        dm = ops.ca_gate_bwd(ds, s, h, m, w1, w2)[0]
        out.append(dict(x=x, t=t, gy=gy, m=m, h=h, s=s, ds=ds, dm=dm, w1=w1, b1=b1, w2=w2, b2=b2))
    return out


def _kernels(sets):
    from pesr_amd import ops
    i = [0]

    def nxt():
        i[0] = (i[0] + 1) % len(sets)
        return sets[i[0]]

    def of(f):
        return lambda: f(nxt())
    return {"pool": of(lambda d: ops.ca_pool(d["t"])),
            "ds": of(lambda d: ops.ca_ds(d["gy"], d["t"], RES_SCALE)),
            "apply_fwd": of(lambda d: ops.ca_apply_fwd(d["x"], d["t"], d["s"], RES_SCALE)),
            "apply_bwd": of(lambda d: ops.ca_apply_bwd(d["gy"], d["s"], d["dm"], RES_SCALE)),
            "gate_fwd": of(lambda d: ops.ca_gate_fwd(d["m"], d["w1"], d["b1"], d["w2"], d["b2"])),
            "gate_bwd": of(lambda d: ops.ca_gate_bwd(d["ds"], d["s"], d["h"], d["m"], d["w1"], d["w2"]))}


def kernels(dev, reps=30, calls=16):
    from pesr_amd import ops
    need = algorithm_bytes()
    out = {"shape": list(SHAPE), "reduction": REDUCTION, "pool_partials": ops.ca_pool_partials(SHAPE[0], SHAPE[1] * SHAPE[2], SHAPE[3]),
           "tensor_MB": round(tensor_bytes() / 1e6, 2), "hbm_TBs": HBM_TBS, "rows": {}}
    for label, count in (("one_set", 1), ("eight_sets", 8)):
        sets = _sets(count, dev)
        for name, fn in _kernels(sets).items():
            us = time_events(fn, reps, 2 * len(sets) * 2, calls=calls)
            gbs = need[name] / us[0] / 1e3
            out["rows"].setdefault(name, {"bytes": need[name]})[label] = {
                "us": us, "GBs": round(gbs, 1), "share_of_hbm": round(gbs / (HBM_TBS * 1e3), 3)}
        del sets
        torch.cuda.empty_cache()
    return out


def steps(dev, reps=12, warmup=3, batch=16, side=192):
    from model import VGG, Discriminator, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    gen = torch.Generator(device="cpu").manual_seed(7)
    hr = torch.randint(0, 256, (batch, 3, side, side), generator=gen).float().to(dev)
    lr = torch.nn.functional.avg_pool2d(hr, 4)
    floor = block_floor_bytes((batch, side // 4, side // 4, 256))
    out = {"batch": batch, "hr_side": side, "blocks": BLOCKS,
           "floor_ms": {k: round(BLOCKS * v / HBM_TBS / 1e9, 3) for k, v in floor.items()},
           "saved_activation_MB": round(BLOCKS * tensor_bytes((batch, side // 4, side // 4, 256)) / 1e6, 1)}
    for phase in ("pretrain", "train"):
        res = {}
        for key, extra in (("off", {}), ("ca", {"attention": "ca", "ca_reduction": REDUCTION})) * 2:
            torch.manual_seed(0)
            opt = dict({"patch_size": side // 4, "num_channels": 256, "depth": BLOCKS, "res_scale": 0.1, "spectral_norm": False, "scale": 4},
                       **extra)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                G = Generator(opt).to(dev)
                D, V = (Discriminator(opt).to(dev), VGG().to(dev)) if phase == "train" else (None, None)
            tr = Trainer(G, D, V, FlatAdam([p for p in G.parameters() if p.requires_grad], lr=1e-6),
                         FlatAdam(D.parameters(), lr=1e-6) if D is not None else None)
            eager = tr.gan_step if phase == "train" else tr.pretrain_step
            for _ in range(3):                                            # first-use work must not happen under capture
                eager(lr, hr)
            run = (tr.capture_gan_step if phase == "train" else tr.capture_pretrain_step)(lr, hr)
            logs = [None]

            def step():
                logs[0] = run(lr, hr)

            t = [round(v / 1e3, 3) for v in time_events(step, reps, warmup)]
            res[key + ("_again" if key in res else "")] = {"ms": t, "logs": {k: round(float(v), 6) for k, v in logs[0].items()}}
            del tr, G, D, V, run, eager
            torch.cuda.empty_cache()
        res["ca_minus_off_ms"] = round((res["ca"]["ms"][0] + res["ca_again"]["ms"][0] - res["off"]["ms"][0] - res["off_again"]["ms"][0]) / 2, 3)
        res["off_spread_ms"] = round(abs(res["off"]["ms"][0] - res["off_again"]["ms"][0]), 3)
        out[phase] = res
    return out


def once(dev):
    """Every kernel twice: after a 512 MB fill that evicts the 256 MiB last-level cache, and again at once.  Dispatch order (for the
    profiler's table): per kernel [fill, cold call, warm call]; pool and ds are two dispatches per call, gate_bwd too."""
    flush = torch.empty(128 * 1024 * 1024, device=dev)
    kernels_ = _kernels(_sets(1, dev))
    torch.cuda.synchronize()
    for fn in kernels_.values():
        flush.zero_()
        fn()
        fn()
    torch.cuda.synchronize()
    return {"ran": list(kernels_), "order": "per kernel: fill, cold call, warm call", "shape": list(SHAPE), "bytes": algorithm_bytes()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "steps", "once", "bytes"])
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if args.what == "bytes":           # (needs no device)
        res = {"kernels": algorithm_bytes(), "block": block_floor_bytes(), "tensor_bytes": tensor_bytes()}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("ca_time.py: no GPU; a time is measured on the MI355X or not at all")
        dev = torch.device("cuda", 0)
        res = {"kernels": kernels, "steps": steps, "once": once}[args.what](dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
