"""Time of the device NIQE block statistics (docs/modes.md section 4k) for one DIV2K-sized image and for a small one.

  python scripts/niqe_time.py [--cases 1356x2040:96,97x131:16] [--shave 0] [--reps 21] [--warmup 3] [--host true]

Per case one JSON line for each of: the C ABI call pesr_niqe_stats (all five launches, no allocation) timed with device events, and
pesr_amd.niqe.niqe_stats as a user calls it (allocates the result) - median / best / worst of --reps runs after --warmup - then the
host feature step (features_from_stats on the sums brought back, wall clock, median of 5; the alpha table is built before) and,
with --host true, the numpy route (stats_numpy) for the same image, once, with a check that the two routes' scores against a model
fitted from the image itself agree.  `rocprofv3 --kernel-trace --stats -- python scripts/niqe_time.py --host false` names the four
kernels apart.  No pass/fail bar.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="1356x2040:96,97x131:16", help="HxW:B, comma-separated")
    ap.add_argument("--shave", type=int, default=0)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", type=lambda x: str(x).lower() == "true", default=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("niqe_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, niqe, ops
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    niqe.alpha_table()
    for case in args.cases.split(","):
        size, B = case.split(":")
        h, w = (int(v) for v in size.split("x"))
        B = int(B)
        g = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
        # smooth shading, 8 x 8 blocks and grain: both signs in every map of every block
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        base = torch.randint(40, 216, (1, 3, (h + 7) // 8, (w + 7) // 8), generator=g).float()
        a = torch.kron(base, torch.ones(8, 8))[:, :, :h, :w] * 0.5 + (0.03 * yy + 0.02 * xx) + 9.0 * torch.randn((1, 3, h, w), generator=g)
        a = a.clamp(0, 255).round()
        da = a.to(dev)
        nby, nbx = niqe.block_grid(h, w, args.shave, B)
        hc, wc = nby * B, nbx * B
        stats = torch.empty((1, 2, nby * nbx, 26), dtype=torch.float64, device=dev)
        ws = ops.workspace(30 * hc * wc, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def abi():
            _lib.check(L.pesr_niqe_stats(da.data_ptr(), 1, h, w, 0, args.shave, B, 0, stats.data_ptr(), None, None, ws.data_ptr(),
                                         ws.numel(), stream), "pesr_niqe_stats")

        res = [None]

        def user():
            res[0] = niqe.niqe_stats(da, args.shave, B, "gray")

        for what, fn in (("pesr_niqe_stats, one call per event pair", abi), ("niqe.niqe_stats (allocates the result)", user)):
            med, best, worst = time_events(fn, args.reps, args.warmup)
            print(json.dumps({"what": what, "image": [h, w], "block": B, "shave": args.shave, "blocks": nby * nbx,
                              "us_median": round(med, 2), "us_best": round(best, 2), "us_worst": round(worst, 2),
                              "workspace_MB": round(30 * hc * wc / 1e6, 2)}), flush=True)
        assert torch.equal(res[0], stats)
        s = stats.cpu().numpy()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            feat = niqe.features_from_stats(s, B)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print(json.dumps({"what": "host feature step (features_from_stats), wall clock", "image": [h, w], "block": B,
                          "fits": 10 * nby * nbx, "ms_median": round(ts[2] * 1e3, 2), "ms_best": round(ts[0] * 1e3, 2),
                          "ms_worst": round(ts[-1] * 1e3, 2)}), flush=True)
        if args.host:
            t0 = time.perf_counter()
            hs = niqe.stats_numpy(a, args.shave, B, "gray")
            dt = time.perf_counter() - t0
            # a model from another image's blocks (a shifted copy), so that the score is not 0
            other = niqe.features_from_stats(niqe.stats_numpy(torch.roll(a, (5, 3), (2, 3)).flip(3), args.shave, B, "gray"), B)
            other = other[np.isfinite(other).all(axis=1)]
            model = niqe.NiqeModel(other.mean(axis=0), np.cov(other, rowvar=False) + 0.01 * np.eye(36), B, "gray", len(other))
            dscore = niqe.score(feat[0], model)
            hscore = niqe.score(niqe.features_from_stats(hs, B), model)
            print(json.dumps({"what": "host float64 numpy route (stats_numpy), one image", "image": [h, w], "block": B,
                              "s_per_image": round(dt, 3), "niqe_host": hscore, "niqe_device": dscore,
                              "rel_diff": abs(hscore - dscore) / hscore}), flush=True)
            assert abs(hscore - dscore) <= 1e-9 * hscore


if __name__ == "__main__":
    main()
