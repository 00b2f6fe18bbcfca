"""Time of the batched bicubic resize (docs/modes.md section 4f) on a synthetic pool of DIV2K-sized images.

  python scripts/resize_time.py [--images 100] [--height 1356] [--width 2040] [--reps 9] [--warmup 2]

For s = 2, 3, 4: the down-resize of the whole pool (height pass, width pass - one launch each through the C ABI, timed separately
with device events - and imresize_pool_u8 as a user calls it, host work included), then the up-resize of the result.  Per
measurement one JSON line: median / best / worst of --reps runs after --warmup, the bytes the pass has to move (input read once +
output written once) over the median time as GB/s and as a share of the MI355X's measured 6.29 TB/s, and the float64 operation
rate (one multiply and one add per tap and output byte).  Last, the host time of the float64 numpy restatement
(tests/resize_oracle.py) for ONE image.  No pass/fail bar: the resize runs once per training run.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.29


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


def report(what, s, up, ms, nbytes, flops, **extra):
    med, best, worst = ms
    row = {"what": what, "s": s, "dir": "up" if up else "down", "ms_median": round(med, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3),
           "MB_moved": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med / 1e6, 1), "share_of_6.29TBs": round(nbytes / med / 1e9 / HBM_TBS, 4)}
    if flops:
        row["fp64_GFLOP_per_s"] = round(flops / med / 1e6, 1)
    row.update(extra)
    print(json.dumps(row), flush=True)


def one_direction(pool, offs, shapes, s, up, reps, warmup):
    """-> (out_pool, out_offsets, out_shapes) after timing both passes and the user-level call."""
    from pesr_amd import _lib
    from pesr_amd.resize import imresize_pool_u8, resize_weights
    L, dev, n = _lib.lib(), pool.device, len(offs)
    taps = 4 if up else {2: 8, 3: 11, 4: 16}[s]
    olen = (lambda v: v * s) if up else (lambda v: v // s)
    mid_shapes = [(olen(h), w) for h, w in shapes]
    out_shapes = [(h, olen(w)) for h, w in mid_shapes]
    cum = lambda shp: np.concatenate([[0], np.cumsum([3 * h * w for h, w in shp])]).astype(np.int64)  # noqa: E731
    in_bytes = sum(3 * h * w for h, w in shapes)
    mid_off, out_off = cum(mid_shapes), cum(out_shapes)
    mid = torch.empty(int(mid_off[-1]), dtype=torch.uint8, device=dev)
    out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
    wts = np.zeros(16)
    w = resize_weights(s, up).reshape(-1)
    wts[:w.size] = w
    stream = torch.cuda.current_stream(dev).cuda_stream
    passes = (("height pass", pool, mid, offs, mid_off, shapes, 0, in_bytes, int(mid_off[-1])),
              ("width pass", mid, out, mid_off, out_off, mid_shapes, 1, int(mid_off[-1]), int(out_off[-1])))
    for what, src, dst, so, do, shp, axis, rd, wr in passes:
        desc = np.array([(int(so[i]), int(do[i]), shp[i][0], shp[i][1]) for i in range(n)], dtype=np.int64)
        ddev = torch.from_numpy(desc).to(dev)

        def run():
            _lib.check(L.pesr_imresize_u8_pass(src.data_ptr(), dst.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), ddev.data_ptr(), n, axis, s,
                                               int(up), wts.ctypes.data_as(ctypes.c_void_p), stream), "pesr_imresize_u8_pass")
        report(what, s, up, time_events(run, reps, warmup), rd + wr, 2 * taps * wr, images=n, taps=taps)
    res = [None]

    def user():
        res[0] = imresize_pool_u8(pool, offs, shapes, s, up)
    report("imresize_pool_u8 (both passes, allocations and descriptor uploads)", s, up, time_events(user, reps, warmup),
           in_bytes + 2 * int(mid_off[-1]) + int(out_off[-1]), 2 * taps * (int(mid_off[-1]) + int(out_off[-1])), images=n)
    assert torch.equal(res[0][0], out)                    # the timed launches computed what the user-level call computes
    return res[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--height", type=int, default=1356)
    ap.add_argument("--width", type=int, default=2040)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    import resize_oracle as RO
    from pesr_amd.resize import modcrop
    for s in (2, 3, 4):
        h, w = args.height - args.height % s, args.width - args.width % s
        torch.manual_seed(s)
        pool = torch.randint(0, 256, (args.images * 3 * h * w,), dtype=torch.uint8, device=dev)
        offs, shapes = [i * 3 * h * w for i in range(args.images)], [(h, w)] * args.images
        lr_pool, lr_off, lr_shapes = one_direction(pool, offs, shapes, s, False, args.reps, args.warmup)
        one_direction(lr_pool, lr_off, lr_shapes, s, True, args.reps, args.warmup)
        # the host restatement on image 0, and a last equality check at full size
        img = pool[:3 * h * w].view(h, w, 3).cpu().numpy()
        t0 = time.perf_counter()
        want = RO.imresize(modcrop(img, s), s, False)
        dt = time.perf_counter() - t0
        ok = bool(torch.equal(lr_pool[:want.size].cpu(), torch.from_numpy(want).reshape(-1)))
        print(json.dumps({"what": "host float64 numpy restatement, one image", "s": s, "dir": "down", "image": [h, w], "s_per_image": round(dt, 3),
                          "device_result_equal": ok}), flush=True)
        assert ok
        del pool, lr_pool
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
