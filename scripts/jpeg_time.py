"""Time of the JPEG round trip (docs/modes.md section 4l) where it is used.

  python scripts/jpeg_time.py [--reps 9] [--warmup 3] [--images 100] [--height 339] [--width 510] [--part ab]

(a) GpuPatchSampler.assemble at B = 16, P = 48, x4 on a pool of 8 DIV2K-sized HR images with a classical DegradationSpec, with and
    without a JPEG range (without: the path of a run without --jpeg_quality, unchanged).  The two are timed alternately, as a user
    calls them - host work, descriptor uploads and allocations included - between device events; the difference is given as a share
    of the 58.7 ms training step.  The pieces on their own: jpeg_pool_u8 on a prepared scratch pool (host work and uploads included),
    and the two launches alone through the C ABI on prepared buffers.
(b) the whole-image form, jpeg_pool_u8 on --images LR images of --height x --width (a DIV2K image at x4), 4:2:0 and 4:4:4; the two
    launches alone too.
Per measurement one JSON line: median / best / worst of --reps runs after --warmup.  The float64 count is 4 passes x 8 multiply-adds
per sample of every coded plane.  The first image of (b) is compared with the host restatement (tests/jpeg_oracle.py).  No pass/fail
bar.
"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from degrade_time import STEP_MS, report, time_alternating, time_events  # noqa: E402


def launch_only(pool, offsets, shapes, strides, qualities, chroma420):
    """-> (callable that issues the two launches through the C ABI on prepared buffers, output tensor)."""
    from pesr_amd import _lib
    from pesr_amd.jpeg import DESC_WORDS, _device_tables, entry_bytes
    n, dev = len(offsets), pool.device
    desc = np.empty((n, DESC_WORDS), dtype=np.int64)
    off = ws_off = 0
    for i in range(n):
        h, w = shapes[i]
        desc[i] = (offsets[i], strides[i], off, w, h, w, qualities[i], ws_off)
        off += 3 * h * w
        ws_off += entry_bytes(h, w, chroma420)
    out = torch.empty(off, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_off, dtype=torch.uint8, device=dev)
    ddev = torch.from_numpy(desc).to(dev)
    T, quant = _device_tables(dev)
    L, stream = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream

    def run():
        _lib.check(L.pesr_jpeg_u8(pool.data_ptr(), out.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), ddev.data_ptr(), n, 420 if chroma420 else 444,
                                  T.data_ptr(), quant.data_ptr(), ws.data_ptr(), ws_off, stream), "pesr_jpeg_u8")
    run.keep = (ddev, desc, ws)
    return run, out


def coded_samples(h, w, chroma420):
    """Samples that go through the four DCT passes: whole 8 x 8 blocks of every plane."""
    up = lambda v: -(-v // 8) * 8
    ch, cw = ((h + 1) // 2, (w + 1) // 2) if chroma420 else (h, w)
    return up(h) * up(w) + 2 * up(ch) * up(cw)


def part_a(args, dev):
    from pesr_amd.degrade import DegradationSpec
    from pesr_amd.input_pipeline import GpuPatchSampler
    from pesr_amd.jpeg import jpeg_pool_u8
    s, B, P = 4, 16, 48
    rng = np.random.default_rng(1)
    hrs = [rng.integers(0, 256, (1356, 2040, 3), dtype=np.uint8) for _ in range(8)]
    with_jpeg = GpuPatchSampler.from_hr(hrs, dev, scale=s, degradation=DegradationSpec(0.8, 4.0, True, 10.0, 30, 95))
    without = GpuPatchSampler.from_hr(hrs, dev, scale=s, degradation=DegradationSpec(0.8, 4.0, True, 10.0))
    picks = with_jpeg.draw(B, P, random.Random(7))
    base = [p[:9] for p in picks]
    t_on, t_off = time_alternating([lambda: with_jpeg.assemble(picks, P, nhwc=True), lambda: without.assemble(base, P, nhwc=True)],
                                   args.reps, args.warmup)
    flops = 2 * 4 * 8 * B * coded_samples(P, P, True)
    m_on = report("(a) assemble, classical degradation + JPEG 4:2:0: B 16, P 48, x4", t_on, fp64_MFLOP=round(flops / 1e6, 1))
    m_off = report("(a) assemble, classical degradation without JPEG (the path of a run without --jpeg_quality)", t_off)
    print(json.dumps({"what": "(a) difference of the medians", "ms": round(m_on - m_off, 4), "share_of_58.7ms_step": round((m_on - m_off) / STEP_MS, 5)}),
          flush=True)
    # the pieces
    scratch = without._degraded_patches(base, P)
    offs, shapes, strides, quals = [3 * P * P * b for b in range(B)], [(P, P)] * B, [P] * B, [p[9] for p in picks]
    report("(a) piece: jpeg_pool_u8 in place on the 16 patches (host work, uploads, workspace)",
           time_events(lambda: jpeg_pool_u8(scratch, offs, shapes, strides, quals, True, out=scratch), args.reps, args.warmup))
    run, _ = launch_only(scratch, offs, shapes, strides, quals, True)
    report("(a) piece: the two launches alone, prepared buffers", time_events(run, args.reps, args.warmup))


def part_b(args, dev):
    import jpeg_oracle as JO
    from pesr_amd.jpeg import jpeg_pool_u8
    n, h, w = args.images, args.height, args.width
    torch.manual_seed(3)
    pool = torch.randint(0, 256, (n * 3 * h * w,), dtype=torch.uint8, device=dev)
    offs, shapes, strides = [i * 3 * h * w for i in range(n)], [(h, w)] * n, [w] * n
    quals = [10 + (83 * i) % 90 for i in range(n)]
    for c420 in (True, False):
        mode = "4:2:0" if c420 else "4:4:4"
        res = [None]

        def user():
            res[0] = jpeg_pool_u8(pool, offs, shapes, strides, quals, c420)
        report(f"(b) jpeg_pool_u8, {n} images of {w} x {h}, {mode}", time_events(user, args.reps, args.warmup))
        run, out = launch_only(pool, offs, shapes, strides, quals, c420)
        med = report(f"(b) the two launches alone, {mode}", time_events(run, args.reps, args.warmup), MB=round(n * 3 * h * w / 1e6, 1))
        flops = 2 * 4 * 8 * n * coded_samples(h, w, c420)
        print(json.dumps({"what": "(b) fp64 rate of the launches alone", "mode": mode, "GFLOP_per_s": round(flops / med / 1e6, 1),
                          "ms_per_image": round(med / n, 4)}), flush=True)
        assert torch.equal(res[0][0], out)
        want = JO.jpeg(pool[:3 * h * w].view(h, w, 3).cpu().numpy(), quals[0], c420)
        ok = bool(torch.equal(out[:want.size].cpu(), torch.from_numpy(want).reshape(-1)))
        print(json.dumps({"what": "host float64 numpy restatement, first image", "mode": mode, "device_result_equal": ok}), flush=True)
        assert ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--height", type=int, default=339)
    ap.add_argument("--width", type=int, default=510)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--part", type=str, default="ab", help="a, b or ab")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    if "a" in args.part:
        part_a(args, dev)
    if "b" in args.part:
        part_b(args, dev)


if __name__ == "__main__":
    main()
