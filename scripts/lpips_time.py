"""Time of the device LPIPS (docs/modes.md section 4n): the five head launches and the whole lpips(), for 16 pairs of 192 x 192 and for
one DIV2K-sized pair.

  python scripts/lpips_time.py [--cases 16x192x192,1x1356x2040] [--reps 21] [--warmup 3] [--burst 20] [--seed 0]

Per case, with LpipsModel.random (the time does not depend on the weights' values) and the features the trunk really produces:
  - per tapped layer one JSON line: the C ABI call pesr_lpips_layer (both kernels, no allocation) in bursts of --burst back-to-back
    calls per device-event pair, divided by their number (launch latency overlapped), median / best / worst of --reps bursts after
    --warmup; the bytes it must read (2 N H W C 4: every feature element once) and that over the median time as a fraction of the
    MI355X's measured 6.29 TB/s; and, measured the same way in the same run, ops.loss_mse (no gradient) on the same two halves of the
    same tensor - the project's plain streaming reduction over the same bytes - with the head's rate over its rate;
  - one line for the trunk alone (LpipsModel.features), one for the whole lpips(), with the head's share of it.
A layer whose features fit the 256 MB Infinity Cache is re-read from there by a burst: its fraction of the HBM rate can exceed 1 and is
marked "cache_resident".  No pass/fail bar.
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS = 6.29
CACHE_BYTES = 256 * 2 ** 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="16x192x192,1x1356x2040", help="NxHxW, comma-separated")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops
    from pesr_amd import lpips as LP
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = LP.LpipsModel.random(args.seed).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for case in args.cases.split(","):
        n, h, w = (int(v) for v in case.split("x"))
        g = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
        a = torch.randint(0, 256, (n, 3, h, w), generator=g).float()
        b = (a + 8.0 * torch.randn(a.shape, generator=g)).clamp(0, 255).round()
        da, db = a.to(dev), b.to(dev)
        x = torch.cat([da, db]).contiguous()
        taps = [t.contiguous() for t in model.features(x)]
        head_us = 0.0
        for l, (f, wt) in enumerate(zip(taps, model.lins)):
            _, fh, fw, c = f.shape
            out = torch.empty(n, dtype=torch.float64, device=dev)
            ws = ops.workspace(8 * n * ((fh * fw + 63) // 64), dev)

            def head():
                _lib.check(L.pesr_lpips_layer(f.data_ptr(), wt.data_ptr(), out.data_ptr(), n, fh, fw, c, None, ws.data_ptr(), ws.numel(), stream),
                           "pesr_lpips_layer")

            fa, fb = f[:n], f[n:]

            def mse():
                ops.loss_mse(fa, fb, 1.0, need_grad=False)

            nbytes = 2 * n * fh * fw * c * 4
            med, best, worst = time_events(head, args.reps, args.warmup, args.burst)
            m_med, m_best, m_worst = time_events(mse, args.reps, args.warmup, args.burst)
            assert torch.equal(out, ops.lpips_layer(f, wt))
            head_us += med
            print(json.dumps({"what": f"pesr_lpips_layer, layer {l}, {args.burst} calls per event pair, per call", "case": [n, h, w],
                              "features": [2 * n, fh, fw, c], "us_median": round(med, 2), "us_best": round(best, 2), "us_worst": round(worst, 2),
                              "read_MB": round(nbytes / 1e6, 2), "us_floor_at_6.29TBs": round(nbytes / HBM_TBS / 1e6, 2),
                              "fraction_of_6.29TBs": round(nbytes / med / 1e6 / HBM_TBS, 3), "cache_resident": nbytes <= CACHE_BYTES,
                              "loss_mse_us_median": round(m_med, 2), "loss_mse_us_best": round(m_best, 2), "loss_mse_us_worst": round(m_worst, 2),
                              "loss_mse_fraction_of_6.29TBs": round(nbytes / m_med / 1e6 / HBM_TBS, 3),
                              "head_rate_over_loss_mse_rate": round(m_med / med, 3)}), flush=True)
        del taps

        res = [None]

        def trunk():
            res[0] = model.features(x)

        def whole():
            res[0] = LP.lpips(da, db, model)

        t_med, t_best, t_worst = time_events(trunk, args.reps, args.warmup)
        w_med, w_best, w_worst = time_events(whole, args.reps, args.warmup)
        print(json.dumps({"what": "LpipsModel.features (input affine, 13 convs, 4 pools), one call per event pair", "case": [n, h, w],
                          "us_median": round(t_med, 1), "us_best": round(t_best, 1), "us_worst": round(t_worst, 1)}), flush=True)
        print(json.dumps({"what": "lpips(), one call per event pair", "case": [n, h, w], "us_median": round(w_med, 1), "us_best": round(w_best, 1),
                          "us_worst": round(w_worst, 1), "five_heads_us_sum_of_medians": round(head_us, 1),
                          "heads_share_of_lpips": round(head_us / w_med, 4), "lpips": [float(v) for v in res[0][:4]]}), flush=True)
        res[0] = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
