"""Time of the classical degradation (docs/modes.md section 4j) where it is used.

  python scripts/degrade_time.py [--reps 9] [--warmup 3] [--images 100] [--height 1356] [--width 2040]

(a) GpuPatchSampler.assemble at B = 16, P = 48, x4 on a pool of 8 DIV2K-sized HR images: with a DegradationSpec whose sigma_hi gives
    K = 24 (per-sample kernels made on the host, one pesr_degrade_u8 launch, two pesr_crop_augment launches) against the bicubic-pool
    sampler (two pesr_crop_augment launches: the path of a run without --degradation classical).  The two are timed alternately, as
    a user calls them - host work, descriptor uploads and allocations included - between device events; the pieces of the
    degradation path are timed on their own as well: the host's kernel bank, and the degrade launch alone through the C ABI.
(b) the whole-image form, degrade_pool_u8 on --images images of --height x --width (mod-cropped) at the widest legal K, for
    s = 2, 3, 4, with and without noise; the launch alone through the C ABI too.
Per measurement one JSON line: median / best / worst of --reps runs after --warmup.  The float64 rate counts one multiply and one add
per tap and output byte.  The first image of (b) is compared with the host restatement (tests/degrade_oracle.py).  No pass/fail bar.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

STEP_MS = 58.7          # the x4 GAN training step this input pipeline feeds (README)


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
    return ts


def time_alternating(fns, reps, warmup):
    """Several callables measured in turn, rep by rep, so that a drift of the machine hits all of them alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k] += time_events(fn, 1, 0)
    return ts


def report(what, ts, **extra):
    ts = sorted(ts)
    row = {"what": what, "ms_median": round(ts[len(ts) // 2], 4), "ms_best": round(ts[0], 4), "ms_worst": round(ts[-1], 4), "runs": len(ts)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return ts[len(ts) // 2]


def launch_only(pool, offsets, shapes, s, bank, kidx, sigmas, qs, windows):
    """-> (callable that issues the one launch through the C ABI on prepared buffers, output tensor)."""
    from pesr_amd import _lib
    from pesr_amd._pool import f64_bits as _f64_bits, i64 as _i64
    from pesr_amd.degrade import DESC_WORDS
    n, dev = len(offsets), pool.device
    desc = np.empty((n, DESC_WORDS), dtype=np.int64)
    off = 0
    for i in range(n):
        y0, x0, h, w = windows[i]
        desc[i] = (offsets[i], off, shapes[i][0], shapes[i][1], y0, x0, h, w, kidx[i], _f64_bits(sigmas[i]), _i64(qs[i]))
        off += 3 * h * w
    out = torch.empty(off, dtype=torch.uint8, device=dev)
    ddev, bdev = torch.from_numpy(desc).to(dev), torch.from_numpy(np.ascontiguousarray(bank)).to(dev)
    L, stream, K = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream, int(bank.shape[1])

    def run():
        _lib.check(L.pesr_degrade_u8(pool.data_ptr(), out.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), ddev.data_ptr(), n, s, K,
                                     bdev.data_ptr(), int(bank.shape[0]), stream), "pesr_degrade_u8")
    run.keep = (ddev, bdev, desc)
    return run, out


def part_a(args, dev):
    from pesr_amd.degrade import DegradationSpec, gaussian_kernel
    from pesr_amd.input_pipeline import GpuPatchSampler
    s, B, P = 4, 16, 48
    rng = np.random.default_rng(1)
    hrs = [rng.integers(0, 256, (1356, 2040, 3), dtype=np.uint8) for _ in range(8)]
    spec = DegradationSpec(0.8, 4.0, True, 10.0)
    blind = GpuPatchSampler.from_hr(hrs, dev, scale=s, degradation=spec)
    plain = GpuPatchSampler.from_hr(hrs, dev, scale=s)
    assert blind.kernel_size == 24
    r = random.Random(7)
    picks = blind.draw(B, P, r)
    base = [p[:4] for p in picks]
    t_blind, t_plain = time_alternating([lambda: blind.assemble(picks, P, nhwc=True), lambda: plain.assemble(base, P, nhwc=True)],
                                        args.reps, args.warmup)
    flops = 2 * 24 * 24 * B * P * P * 3
    m_blind = report("(a) assemble, classical degradation: B 16, P 48, x4, K 24, aniso, noise", t_blind, fp64_MFLOP=round(flops / 1e6, 1))
    m_plain = report("(a) assemble, bicubic LR pool (the default path)", t_plain)
    print(json.dumps({"what": "(a) difference of the medians", "ms": round(m_blind - m_plain, 4),
                      "share_of_58.7ms_step": round((m_blind - m_plain) / STEP_MS, 5), "classical_share_of_58.7ms_step": round(m_blind / STEP_MS, 5)}),
          flush=True)
    # the pieces
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        bank = np.stack([gaussian_kernel(24, p[4], p[5], p[6]) for p in picks])
        host.append((time.perf_counter() - t0) * 1e3)
    report("(a) piece: 16 Gaussian kernels of 24 x 24 on the host (perf_counter)", host)
    run, _ = launch_only(blind.hr_pool, [blind.hr_off[p[0]] for p in picks], [blind.hr_shapes[p[0]] for p in picks], s, bank, list(range(B)),
                         [p[7] for p in picks], [p[8] for p in picks], [(p[1], p[2], P, P) for p in picks])
    med = report("(a) piece: the pesr_degrade_u8 launch alone, prepared buffers", time_events(run, args.reps, args.warmup))
    print(json.dumps({"what": "(a) piece: fp64 rate of that launch", "GFLOP_per_s": round(flops / med / 1e6, 1)}), flush=True)
    lr, _ = blind.assemble(picks, P, nhwc=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        blind.assemble(picks, P, nhwc=True)
    torch.cuda.synchronize()
    print(json.dumps({"what": "(a) classical assemble, host clock over 20 calls ending in a synchronise", "ms_per_call":
                      round((time.perf_counter() - t0) * 50, 4)}), flush=True)


def part_b(args, dev):
    import degrade_oracle as DO
    from pesr_amd.degrade import degrade_pool_u8, gaussian_kernel
    n = args.images
    for s in (2, 3, 4):
        K = 24 if s % 2 == 0 else 23
        h, w = args.height - args.height % s, args.width - args.width % s
        torch.manual_seed(s)
        pool = torch.randint(0, 256, (n * 3 * h * w,), dtype=torch.uint8, device=dev)
        offs, shapes = [i * 3 * h * w for i in range(n)], [(h, w)] * n
        kern = gaussian_kernel(K, K / 6.0, K / 15.0, 0.6)
        out_bytes = n * 3 * (h // s) * (w // s)
        flops = 2 * K * K * out_bytes
        for sigma in (0.0, 30.0):
            res = [None]

            def user():
                res[0] = degrade_pool_u8(pool, offs, shapes, s, kern[None], [0] * n, [sigma] * n, list(range(n)))
            med = report(f"(b) degrade_pool_u8, {n} images of {w} x {h}, x{s}, K {K}, sigma_n {sigma}", time_events(user, args.reps, args.warmup))
            run, out = launch_only(pool, offs, shapes, s, kern[None], [0] * n, [sigma] * n, list(range(n)), [(0, 0, h // s, w // s)] * n)
            med = report("(b) the launch alone", time_events(run, args.reps, args.warmup), MB_in=round(n * 3 * h * w / 1e6, 1),
                         MB_out=round(out_bytes / 1e6, 1))
            print(json.dumps({"what": "(b) fp64 rate of the launch alone", "s": s, "K": K, "sigma_n": sigma, "TFLOP_per_s": round(flops / med / 1e9, 2),
                              "ms_per_image": round(med / n, 4)}), flush=True)
            assert torch.equal(res[0][0], out)
            img = pool[:3 * h * w].view(h, w, 3).cpu().numpy()
            t0 = time.perf_counter()
            want = DO.degrade(img, s, kern, sigma, 0)
            dt = time.perf_counter() - t0
            ok = bool(torch.equal(out[:want.size].cpu(), torch.from_numpy(want).reshape(-1)))
            print(json.dumps({"what": "host float64 numpy restatement, one image", "s": s, "sigma_n": sigma, "s_per_image": round(dt, 3),
                              "device_result_equal": ok}), flush=True)
            assert ok
        del pool
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--height", type=int, default=1356)
    ap.add_argument("--width", type=int, default=2040)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--part", type=str, default="ab", help="a, b or ab")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    if "a" in args.part:
        part_a(args, dev)
    if "b" in args.part:
        part_b(args, dev)


if __name__ == "__main__":
    main()
