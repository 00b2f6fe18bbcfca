"""Time of the any-size resize (docs/modes.md section 4m) and of the resize jitter in the training sampler.

  python scripts/resize_to_time.py [--what pool,patches] [--images 100] [--height 1356] [--width 2040] [--ratio 0.37] [--jitter 0.5,2]
                                   [--reps 9] [--warmup 2] [--tree DIR]

pool: a synthetic pool of DIV2K-sized images resized to --ratio of their sides, per filter: the height pass and the width pass (one
launch each through the C ABI, timed separately with device events) and imresize_to_pool_u8 as a user calls it, host work included.
Per measurement one JSON line: median / best / worst of --reps runs after --warmup, the taps of the pass, taps x output bytes (what
section 4f's per-tap rates are counted in) and that over the median time, the bytes moved (input read once + output written once)
as GB/s.
patches: GpuPatchSampler._degraded_patches at B = 16, P = 48, x4 - a step's LR patches - without and with a resize jitter, on the same
picks up to the jitter's own three values; device events around the call (they span the host work between its launches) and the
wall time of the call ended by a synchronise.  --tree DIR takes pesr_amd from another checkout of the project (for instance the
parent commit, which has no jitter: only the call without it is then timed).
No pass/fail bar.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--what", type=str, default="pool,patches")
ap.add_argument("--images", type=int, default=100)
ap.add_argument("--height", type=int, default=1356)
ap.add_argument("--width", type=int, default=2040)
ap.add_argument("--ratio", type=float, default=0.37)
ap.add_argument("--jitter", type=str, default="0.5,2")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tree", type=str, default="")
ARGS = ap.parse_args()

ROOT = os.path.abspath(ARGS.tree) if ARGS.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def time_events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def time_wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return {"ms_median": round(t[0], 3), "ms_best": round(t[1], 3), "ms_worst": round(t[2], 3)}


def pool_part(dev):
    from pesr_amd import _lib
    from pesr_amd.resize import METHODS, imresize_to_pool_u8, resize_to_plan
    from pesr_amd.degrade import jitter_size
    L, n, h, w = _lib.lib(), ARGS.images, ARGS.height, ARGS.width
    ho, wo = jitter_size(h, ARGS.ratio), jitter_size(w, ARGS.ratio)
    torch.manual_seed(1)
    pool = torch.randint(0, 256, (n * 3 * h * w,), dtype=torch.uint8, device=dev)
    offs, shapes, outs = [i * 3 * h * w for i in range(n)], [(h, w)] * n, [(ho, wo)] * n
    stream = torch.cuda.current_stream(dev).cuda_stream
    for m in METHODS:
        buf, descs, mid_bytes, out_off, _ = resize_to_plan(offs, shapes, outs, [m] * n, [w] * n, [0.0] * n, [0] * n)
        buf_dev = torch.from_numpy(buf).to(dev)
        mid = torch.empty(mid_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
        for axis, (what, src, dst, rd, wr) in enumerate((("height pass", pool, mid, pool.numel(), mid_bytes),
                                                          ("width pass", mid, out, mid_bytes, int(out_off[-1])))):
            desc = descs[axis]
            ddev = torch.from_numpy(desc).to(dev)
            taps = int(desc[0, 9])

            def run():
                _lib.check(L.pesr_resize_to_u8_pass(src.data_ptr(), dst.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), ddev.data_ptr(), n, axis,
                                                    buf_dev.data_ptr(), int(buf.size), stream), "pesr_resize_to_u8_pass")
            t = time_events(run, ARGS.reps, ARGS.warmup)
            row = {"what": what, "filter": m, "images": n, "from": [h, w], "to": [ho, wo], "taps": taps, "taps_x_output_MB": round(taps * wr / 1e6, 1),
                   "G_tap_bytes_per_s": round(taps * wr / t[0] / 1e6, 1), "MB_moved": round((rd + wr) / 1e6, 1),
                   "GB_per_s": round((rd + wr) / t[0] / 1e6, 1)}
            row.update(ms(t))
            print(json.dumps(row), flush=True)
        res = [None]

        def user():
            res[0] = imresize_to_pool_u8(pool, offs, shapes, outs, m)
        row = {"what": "imresize_to_pool_u8 (both passes, tables, allocations and uploads)", "filter": m, "images": n}
        row.update(ms(time_events(user, ARGS.reps, ARGS.warmup)))
        print(json.dumps(row), flush=True)
        assert torch.equal(res[0][0], out)                    # the timed launches computed what the user-level call computes
        del mid, out, res


def patches_part(dev):
    from pesr_amd.degrade import DegradationSpec
    from pesr_amd.input_pipeline import GpuPatchSampler
    B, P, s = 16, 48, 4
    rng = np.random.default_rng(3)
    hrs = [rng.integers(0, 256, (512, 640, 3), dtype=np.uint8) for _ in range(8)]
    plain = DegradationSpec(0.8, 3.2, True, 10.0)
    samp = GpuPatchSampler.from_hr(hrs, dev, scale=s, degradation=plain)
    picks = samp.draw(B, P, random.Random(1))
    runs = [("without jitter", samp, picks)]
    if hasattr(plain, "jitter_hi"):
        lo, hi = (float(v) for v in ARGS.jitter.split(","))
        spec = DegradationSpec(0.8, 3.2, True, 10.0, 0, 0, True, lo, hi)
        r = random.Random(2)
        runs.append((f"with jitter {lo},{hi}", GpuPatchSampler.from_hr(hrs, dev, scale=s, degradation=spec),
                     [p + (r.uniform(lo, hi), r.randrange(3), r.randrange(3)) for p in picks]))
    for tag, sm, pk in runs * 2:                              # each twice, alternating
        fn = lambda: sm._degraded_patches(pk, P)  # noqa: E731
        row = {"what": "_degraded_patches B=16 P=48 x4", "case": tag, "tree": ROOT}
        row.update({"events_" + k: v for k, v in ms(time_events(fn, ARGS.reps, ARGS.warmup)).items()})
        row.update({"wall_" + k: v for k, v in ms(time_wall(fn, ARGS.reps, ARGS.warmup)).items()})
        print(json.dumps(row), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("resize_to_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    for part in ARGS.what.split(","):
        {"pool": pool_part, "patches": patches_part}[part](dev)


if __name__ == "__main__":
    main()
