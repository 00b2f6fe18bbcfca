"""Time of LPIPS as a training loss (docs/modes.md section 4o) at the training shape, 16 pairs of 192 x 192.

  python scripts/lpips_loss_time.py [--case 16x192x192] [--reps 21] [--warmup 3] [--burst 20] [--seed 0]

With LpipsModel.random (the time does not depend on the weights' values) and the features the trunk really produces:
  - per tapped layer one JSON line: the C ABI call pesr_lpips_layer_bwd (one kernel, no allocation) in bursts of --burst back-to-back
    calls per device-event pair, divided by their number (launch latency overlapped), median / best / worst of --reps bursts after
    --warmup, beside its STREAMING BOUND: the bytes it must move (3 N H W C 4: two feature tensors read, one gradient written) at the
    MI355X's measured 6.29 TB/s.  The ratio says whether the float64 arithmetic - two divisions per element - or the memory system
    limits the kernel.  The forward pesr_lpips_layer2 on the same tensors is timed the same way beside it;
  - one line for the whole loss: lpips_loss(sr, hr).mean() forward, and forward plus backward to sr, in milliseconds per step, with the
    five head gradients' share.
A layer whose three tensors fit the 256 MB Infinity Cache is re-read from there by a burst: its fraction of the HBM rate can exceed 1
and is marked "cache_resident".  No pass/fail bar.
"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from _loss_time import HBM_TBS, time_events  # noqa: E402  (puts the repository root on sys.path)

CACHE_BYTES = 256 * 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=str, default="16x192x192", help="NxHxW, both sides multiples of 16")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_loss_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops
    from pesr_amd import lpips as LP
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = LP.LpipsModel.random(args.seed).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, h, w = (int(v) for v in args.case.split("x"))
    why = LP.check_loss_side(h, w)
    if why:
        raise SystemExit(f"lpips_loss_time.py: --case {args.case}: {why}")
    g = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
    hr = torch.randint(0, 256, (n, 3, h, w), generator=g).float()
    sr = (hr + 8.0 * torch.randn(hr.shape, generator=g)).clamp(0, 255)
    dsr, dhr = sr.to(dev).contiguous(memory_format=torch.channels_last), hr.to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        taps_a = [t.contiguous() for t in model.features_grad(dsr)]
        taps_b = [t.contiguous() for t in model.features_grad(dhr)]
    gout = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
    bwd_us = 0.0
    for l, (fa, fb, wt) in enumerate(zip(taps_a, taps_b, model.lins)):
        _, fh, fw, c = fa.shape
        ga = torch.empty_like(fa)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        ws = ops.workspace(8 * n * ((fh * fw + 63) // 64), dev)

        def bwd():
            _lib.check(L.pesr_lpips_layer_bwd(fa.data_ptr(), fb.data_ptr(), wt.data_ptr(), gout.data_ptr(), ga.data_ptr(), n, fh, fw, c, stream),
                       "pesr_lpips_layer_bwd")

        def fwd():
            _lib.check(L.pesr_lpips_layer2(fa.data_ptr(), fb.data_ptr(), wt.data_ptr(), out.data_ptr(), n, fh, fw, c, None, ws.data_ptr(),
                                           ws.numel(), stream), "pesr_lpips_layer2")

        nbytes = 3 * n * fh * fw * c * 4
        med, best, worst = time_events(bwd, args.reps, args.warmup, args.burst, digits=None)
        f_med, f_best, f_worst = time_events(fwd, args.reps, args.warmup, args.burst, digits=None)
        assert torch.equal(ga, ops.lpips_layer_bwd(fa, fb, wt, gout))
        bwd_us += med
        bound = nbytes / HBM_TBS / 1e6
        print(json.dumps({"what": f"pesr_lpips_layer_bwd, layer {l}, {args.burst} calls per event pair, per call", "case": [n, h, w],
                          "features": [n, fh, fw, c], "us_median": round(med, 2), "us_best": round(best, 2), "us_worst": round(worst, 2),
                          "moved_MB": round(nbytes / 1e6, 2), "us_streaming_bound_at_6.29TBs": round(bound, 2),
                          "time_over_streaming_bound": round(med / bound, 2), "fraction_of_6.29TBs": round(bound / med, 3),
                          "cache_resident": nbytes <= CACHE_BYTES, "elements_per_us": round(n * fh * fw * c / med, 1),
                          "forward_us_median": round(f_med, 2), "forward_us_best": round(f_best, 2), "forward_us_worst": round(f_worst, 2),
                          "forward_fraction_of_6.29TBs": round(2 * nbytes / 3 / f_med / 1e6 / HBM_TBS, 3)}), flush=True)
    del taps_a, taps_b

    res = [None]

    def forward():
        with torch.no_grad():
            res[0] = LP.lpips_loss(dsr, dhr, model).mean()

    def both():
        x = dsr.detach().requires_grad_()
        loss = LP.lpips_loss(x, dhr, model).mean()
        loss.backward()
        res[0] = loss.detach()

    def metric():
        res[0] = LP.lpips(dsr, dhr, model).mean()

    f_med, f_best, f_worst = time_events(forward, args.reps, args.warmup, digits=None)
    b_med, b_best, b_worst = time_events(both, args.reps, args.warmup, digits=None)
    m_med, m_best, m_worst = time_events(metric, args.reps, args.warmup, digits=None)
    print(json.dumps({"what": "lpips_loss(sr, hr).mean(): forward alone (no graph); forward + backward to sr; lpips() for comparison; one "
                              "call per event pair", "case": [n, h, w],
                      "forward_ms_median": round(f_med / 1e3, 3), "forward_ms_best": round(f_best / 1e3, 3), "forward_ms_worst": round(f_worst / 1e3, 3),
                      "forward_backward_ms_median": round(b_med / 1e3, 3), "forward_backward_ms_best": round(b_best / 1e3, 3),
                      "forward_backward_ms_worst": round(b_worst / 1e3, 3), "lpips_metric_ms_median": round(m_med / 1e3, 3),
                      "five_head_gradients_us_sum_of_medians": round(bwd_us, 1),
                      "head_gradients_share_of_forward_backward": round(bwd_us / b_med, 4), "loss": float(res[0])}), flush=True)


if __name__ == "__main__":
    main()
