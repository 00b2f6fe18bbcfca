"""Time of SSIM-Y as a training loss (docs/modes.md section 4p) at the training shapes, 16 pairs of 192 x 192 and of 96 x 96.

  python scripts/ssim_loss_time.py [--cases 16x192x192,16x96x96] [--reps 21] [--warmup 3] [--burst 20] [--step]

Per case and per layout of sr (channels_last as the Generator gives it, and NCHW) one JSON line: the C ABI calls pesr_ssim_loss_fwd
(with and without the coefficient maps) and pesr_ssim_loss_bwd, no allocation, in bursts of --burst back-to-back calls per device-event
pair, divided by their number (launch latency overlapped): median / best / worst of --reps bursts after --warmup, beside their
STREAMING BOUNDS at the MI355X's measured 6.29 TB/s - forward: both images read, coef written; backward: both images and coef read,
the gradient written.  At these sizes everything fits the Infinity Cache, so a burst re-reads from there: the bound is a scale, not a
limit the kernels could reach from HBM.  Then ssim_loss(sr, hr).mean() forward + backward through autograd, one call per event pair.
--step: also Trainer.pretrain_step of the full-size Generator with the term off and on, two trainers each, alternating.
No pass/fail bar.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from _loss_time import HBM_TBS, step_ab, time_events  # noqa: E402  (puts the repository root on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="16x192x192,16x96x96", help="comma-separated NxHxW")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time Trainer.pretrain_step of the full-size Generator with the term off and on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_loss_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops
    from pesr_amd import functional as PF
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for case in args.cases.split(","):
        n, h, w = (int(v) for v in case.split("x"))
        gen = torch.Generator(device="cpu").manual_seed(h * 10007 + w)
        hr = torch.randint(0, 256, (n, 3, h, w), generator=gen).float()
        sr = hr + 8.0 * torch.randn(hr.shape, generator=gen)
        ho, wo = h - 10, w - 10
        score = torch.empty(n, dtype=torch.float64, device=dev)
        coef = torch.empty((n, 3, ho, wo), dtype=torch.float64, device=dev)
        gout = torch.full((n,), -1.0 / n, dtype=torch.float64, device=dev)
        ws = ops.workspace(8 * n * ((ho + 15) // 16) * ((wo + 15) // 16), dev)
        img_bytes, coef_bytes = n * 3 * h * w * 4, n * 3 * ho * wo * 8
        for nhwc in (1, 0):
            fmt = torch.channels_last if nhwc else torch.contiguous_format
            dsr, dhr = sr.to(dev).contiguous(memory_format=fmt), hr.to(dev).contiguous(memory_format=torch.channels_last)
            ga = torch.empty_like(dsr)

            def fwd(c=coef.data_ptr()):
                _lib.check(L.pesr_ssim_loss_fwd(dsr.data_ptr(), dhr.data_ptr(), score.data_ptr(), n, h, w, nhwc, 1, c, ws.data_ptr(),
                                                ws.numel(), stream), "pesr_ssim_loss_fwd")

            def bwd():
                _lib.check(L.pesr_ssim_loss_bwd(dsr.data_ptr(), dhr.data_ptr(), coef.data_ptr(), gout.data_ptr(), ga.data_ptr(), n, h, w,
                                                nhwc, 1, stream), "pesr_ssim_loss_bwd")

            def both():
                x = dsr.detach().requires_grad_()
                PF.ssim_loss(x, dhr).mean().backward()

            t_fwd = time_events(fwd, args.reps, args.warmup, args.burst)
            t_score = time_events(lambda: fwd(None), args.reps, args.warmup, args.burst)
            fwd()
            t_bwd = time_events(bwd, args.reps, args.warmup, args.burst)
            assert torch.equal(ga, ops.ssim_loss_bwd(dsr, dhr, coef, gout))
            t_both = time_events(both, args.reps, args.warmup)
            b_fwd, b_bwd = (2 * img_bytes + coef_bytes) / HBM_TBS / 1e6, (3 * img_bytes + coef_bytes) / HBM_TBS / 1e6
            print(json.dumps({"case": [n, h, w], "sr_layout": "NHWC" if nhwc else "NCHW", "calls_per_event_pair": args.burst,
                              "fwd_with_coef_us_median_best_worst": t_fwd, "fwd_score_only_us_median_best_worst": t_score,
                              "bwd_us_median_best_worst": t_bwd, "coef_MB": round(coef_bytes / 1e6, 2),
                              "fwd_us_streaming_bound_at_6.29TBs": round(b_fwd, 2), "bwd_us_streaming_bound_at_6.29TBs": round(b_bwd, 2),
                              "fwd_time_over_bound": round(t_fwd[0] / b_fwd, 1), "bwd_time_over_bound": round(t_bwd[0] / b_bwd, 1),
                              "autograd_forward_backward_us_median_best_worst_one_call_per_pair": t_both,
                              "score_mean": float(score.mean())}), flush=True)
    if args.step:
        pretrain_step_times(args, dev)


def pretrain_step_times(args, dev):
    """Trainer.pretrain_step of the full-size Generator (256 channels, 32 blocks, batch 16, LR 48 x 48 -> HR 192 x 192) with the term off
    and on: ms per step, median of --reps single steps after --warmup; both twice, alternating (_loss_time.step_ab)."""
    out = {"what": "Trainer.pretrain_step, 256 ch x 32 blocks, batch 16, 48 -> 192: ms per step [median, best, worst]"}
    out.update(step_ab([(f"alpha_ssim_{alpha:g}", {"alpha_ssim": alpha}) for alpha in (0.0, 1.0)], dev, 16, 192, args.reps, args.warmup,
                       phase="pretrain"))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
