"""Time of the device DISTS (docs/modes.md section 4t) beside LPIPS of the same pairs: one 192 x 192 pair and one 512 x 512 pair.

  python scripts/dists_time.py [--cases 1x192x192,1x512x512] [--reps 21] [--warmup 3] [--burst 20] [--seed 0]

Per case, with DistsModel.random and LpipsModel.random (the time does not depend on the weights' values) and the features the trunk
really produces, the timer of scripts/_loss_time.py (device events, a warm-up first, median / best / worst of --reps):
  - per stage one JSON line: ops.dists_layer (five launches: two passes over the features, two mean_partials, the score) in bursts of
    --burst back-to-back calls per event pair, divided by their number; the bytes it must read (2 passes x 2 N H W C 4);
  - per pool one line: ops.l2pool_fwd on the trunk's own tensor, the same way (its output allocation included);
  - one line each for dists() and lpips(), one call per event pair, with the share of the two new kernels' launches in dists().
No pass/fail bar.
"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _loss_time import time_events  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="1x192x192,1x512x512", help="NxHxW, comma-separated")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dists_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops
    from pesr_amd import dists as DS
    from pesr_amd import lpips as LP
    dev = torch.device("cuda")
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dmodel = DS.DistsModel.random(args.seed).to(dev)
        lmodel = LP.LpipsModel.random(args.seed).to(dev)
    aw, bw = dmodel.normalised(dev)
    for case in args.cases.split(","):
        n, h, w = (int(v) for v in case.split("x"))
        g = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
        a = torch.randint(0, 256, (n, 3, h, w), generator=g).float()
        b = (a + 8.0 * torch.randn(a.shape, generator=g)).clamp(0, 255).round()
        da, db = a.to(dev), b.to(dev)
        x = torch.cat([da, db]).contiguous()
        stages = [t.contiguous() for t in dmodel.features(x)]
        new_us, c0 = 0.0, 0
        for s, f in enumerate(stages):
            _, fh, fw, c = f.shape
            al, be = aw[c0:c0 + c], bw[c0:c0 + c]
            c0 += c
            med, best, worst = time_events(lambda: ops.dists_layer(f, al, be), args.reps, args.warmup, args.burst)
            new_us += med
            print(json.dumps({"what": f"ops.dists_layer, stage {s}, {args.burst} calls per event pair, per call", "case": [n, h, w],
                              "features": [2 * n, fh, fw, c], "pixel_blocks": ops.dists_plan(n, fh * fw, c)["pixel_blocks"],
                              "us_median": med, "us_best": best, "us_worst": worst, "read_MB": round(2 * 2 * n * fh * fw * c * 4 / 1e6, 3)}),
                  flush=True)
        for s in (1, 2, 3, 4):                                          # the pool behind stage s reads that stage's tensor
            f = stages[s]
            _, fh, fw, c = f.shape
            med, best, worst = time_events(lambda: ops.l2pool_fwd(f), args.reps, args.warmup, args.burst)
            new_us += med
            print(json.dumps({"what": f"ops.l2pool_fwd behind stage {s}, {args.burst} calls per event pair, per call", "case": [n, h, w],
                              "input": [2 * n, fh, fw, c], "us_median": med, "us_best": best, "us_worst": worst,
                              "read_and_written_MB": round(2 * n * c * 4 * (fh * fw + ((fh + 1) // 2) * ((fw + 1) // 2)) / 1e6, 3)}), flush=True)
        del stages
        res = [None]

        def run_dists():
            res[0] = DS.dists(da, db, dmodel)

        def run_lpips():
            res[0] = LP.lpips(da, db, lmodel)

        d_med, d_best, d_worst = time_events(run_dists, args.reps, args.warmup, 1, 1)
        score = [float(v) for v in res[0]]
        l_med, l_best, l_worst = time_events(run_lpips, args.reps, args.warmup, 1, 1)
        d2 = time_events(run_dists, args.reps, args.warmup, 1, 1)       # again, behind LPIPS: the spread between two windows
        print(json.dumps({"what": "dists(), one call per event pair", "case": [n, h, w], "us_median": d_med, "us_best": d_best, "us_worst": d_worst,
                          "us_median_again": d2[0], "new_kernels_us_sum_of_medians": round(new_us, 1),
                          "new_kernels_share_of_dists": round(new_us / d_med, 4), "dists": score}), flush=True)
        print(json.dumps({"what": "lpips(), one call per event pair", "case": [n, h, w], "us_median": l_med, "us_best": l_best, "us_worst": l_worst,
                          "dists_over_lpips": round(d_med / l_med, 3)}), flush=True)
        res[0] = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
