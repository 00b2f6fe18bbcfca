"""Time of the device SSIM-Y (docs/modes.md section 4g) for one DIV2K-sized pair and for a small one.

  python scripts/ssim_time.py [--sizes 1356x2040,97x131] [--shave 4] [--reps 21] [--warmup 3] [--burst 50] [--host true]

Per size one JSON line for each of: the C ABI call (both kernels, no allocation) timed with device events one call at a time, the
same in a burst of --burst back-to-back calls divided by their number (launch latency overlapped: the closest a device event gets
to the kernels' own time; `rocprofv3 --kernel-trace --stats -- python scripts/ssim_time.py --host false` names them apart), and
ops.ssim_y as a user calls it.  Each gives median / best / worst of --reps runs after --warmup, and beside it the floor of reading
both inputs once at the MI355X's measured 6.29 TB/s and the float64 operations the algorithm needs over the median time.  With
--host true also the host float64 route (utils.compute_SSIM on CPU tensors) for the same pair, once, and a check that the device
result agrees with it.  The tile size is fixed when the library is built; PESR_HIP_LIB=<another build> times an alternative.
No pass/fail bar.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS = 6.29


def time_events(fn, reps, warmup, calls=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def fp64_ops(h, w, shave):
    """Multiplies, adds and divisions of the definition per pair, each filtered value computed once: 3 products per pixel, two
    passes of 5 maps x 11 taps x (mul + add), 21 operations for the map value (the division counted as one)."""
    hs, ws = h - 2 * shave, w - 2 * shave
    ho, wo = hs - 10, ws - 10
    return 3 * hs * ws + 5 * 11 * 2 * ho * ws + 5 * 11 * 2 * ho * wo + 21 * ho * wo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="1356x2040,97x131")
    ap.add_argument("--shave", type=int, default=4)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--host", type=lambda x: str(x).lower() == "true", default=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops
    import utils
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
        a = torch.randint(0, 256, (1, 3, h, w), generator=g).float()
        b = (a + 8.0 * torch.randn(a.shape, generator=g)).clamp(0, 255).round()
        da, db = a.to(dev), b.to(dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        ho, wo = h - 2 * args.shave - 10, w - 2 * args.shave - 10
        ws = ops.workspace(8 * ((ho + 15) // 16) * ((wo + 15) // 16), dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def abi():
            _lib.check(L.pesr_ssim_y(da.data_ptr(), db.data_ptr(), out.data_ptr(), 1, h, w, 0, 0, args.shave, None, ws.data_ptr(), ws.numel(),
                                     stream), "pesr_ssim_y")

        res = [None]

        def user():
            res[0] = ops.ssim_y(da, db, args.shave)

        in_bytes = 2 * 3 * 4 * h * w
        flops = fp64_ops(h, w, args.shave)
        for what, fn, calls in (("pesr_ssim_y, one call per event pair", abi, 1),
                                (f"pesr_ssim_y, {args.burst} calls per event pair, per call", abi, args.burst),
                                ("ops.ssim_y (allocates the result)", user, 1)):
            med, best, worst = time_events(fn, args.reps, args.warmup, calls)
            print(json.dumps({"what": what, "image": [h, w], "shave": args.shave, "us_median": round(med, 2), "us_best": round(best, 2),
                              "us_worst": round(worst, 2), "input_MB": round(in_bytes / 1e6, 2),
                              "us_floor_inputs_once_at_6.29TBs": round(in_bytes / HBM_TBS / 1e6, 2),
                              "fp64_Gop": round(flops / 1e9, 4), "fp64_Top_per_s": round(flops / med / 1e6, 3)}), flush=True)
        assert torch.equal(res[0], out)
        if args.host:
            t0 = time.perf_counter()
            host = utils.compute_SSIM(a, b, args.shave)
            dt = time.perf_counter() - t0
            print(json.dumps({"what": "host float64 numpy route (utils.compute_SSIM on CPU tensors), one pair", "image": [h, w],
                              "s_per_pair": round(dt, 3), "host": host, "device": float(out[0]), "abs_diff": abs(host - float(out[0]))}),
                  flush=True)
            assert abs(host - float(out[0])) <= 1e-9


if __name__ == "__main__":
    main()
