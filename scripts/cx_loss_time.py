"""Time of the contextual loss's kernels (docs/modes.md section 4r) at the training shape: batch 16, HR 192 x 192, so the relu3_4 tap is
[16, 48, 48, 256]: P = 2304 points per image, D is [16, 2304, 2304] (340 MB).

  python scripts/cx_loss_time.py [--batch 16] [--side 192] [--reps 21] [--warmup 3] [--burst 5] [--step]

One JSON line: the C ABI calls pesr_cx_normalize, pesr_cx_dist, pesr_cx_fwd and pesr_cx_bwd, no allocation, in bursts of --burst
back-to-back calls per device-event pair, divided by their number: median / best / worst of --reps bursts after --warmup.  Beside each
its FLOOR, the larger of bytes moved / 6.29 TB/s and issued FLOPs / 157.3 TFLOP/s, and the fraction of the floor reached (floor / time).
Bytes, each array counted once however often a kernel reads it: normalise fa, fb read and xh, yh written; distance xh, yh read and D
written; forward D read; backward D, xh, yh read and the gradient written.  FLOPs: 2 P P C per image for each of the two GEMMs.
--step: the captured Trainer.gan_step of the full-size networks (bench.py's: 256 channels x 32 blocks, batch 16, 48 -> 192) with the
term off and on, two trainers each, alternating: ms per step.  No pass/fail bar.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from _loss_time import floor_us, step_ab, time_events  # noqa: E402  (puts the repository root on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=192, help="the HR side: the tap is side / 4")
    ap.add_argument("--h", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time Trainer.gan_step of the full-size networks with the term off and on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cx_loss_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, contextual, ops
    why = contextual.check_size(args.side, args.side)
    if why:
        raise SystemExit(f"cx_loss_time.py: {why}")
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, c = args.batch, contextual.TAP_CHANNELS
    th, tw = contextual.tap_size(args.side, args.side)
    P = th * tw
    plan = ops.cx_plan(n, P, c)
    gen = torch.Generator(device="cpu").manual_seed(P * 10007 + c)
    fb = torch.randn((n, th, tw, c), generator=gen).add_(0.3).relu_()
    fa = (fb + torch.randn((n, th, tw, c), generator=gen)).relu_().to(dev)
    fb = fb.to(dev)
    xh, yh, inv, mu = ops.cx_normalize(fa, fb)
    D, m, b = ops.cx_dist(xh, yh)
    Lv, CX, S, a, cmax = ops.cx_fwd(D, m, args.h, c)
    gf = torch.empty_like(fa)
    gout = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
    ws = ops.workspace(plan["workspace_bytes"], dev)
    p = lambda t: t.data_ptr()

    def normalize():
        _lib.check(L.pesr_cx_normalize(p(fa), p(fb), p(mu), p(xh), p(yh), p(inv), n, P, c, stream), "pesr_cx_normalize")

    def dist():
        _lib.check(L.pesr_cx_dist(p(xh), p(yh), p(D), p(m), p(b), n, P, c, stream), "pesr_cx_dist")

    def fwd():
        _lib.check(L.pesr_cx_fwd(p(D), p(m), args.h, p(S), p(a), p(cmax), p(CX), p(Lv), n, P, c, p(ws), ws.numel(), stream), "pesr_cx_fwd")

    def bwd():
        _lib.check(L.pesr_cx_bwd(p(D), p(m), p(b), p(S), p(a), p(cmax), p(CX), p(gout), p(xh), p(yh), p(inv), args.h, p(gf), None, None,
                                 n, P, c, p(ws), ws.numel(), stream), "pesr_cx_bwd")

    f_bytes, d_bytes, gemm = fa.numel() * 4, D.numel() * 4, 2.0 * P * P * c * n
    out = {"tap": [n, th, tw, c], "points": P, "plan": plan, "calls_per_event_pair": args.burst, "D_MB": round(d_bytes / 1e6, 1),
           "F_MB": round(f_bytes / 1e6, 2), "gemm_GFLOP": round(gemm / 1e9, 2)}
    total = 0.0
    for name, fn, fl in (("normalize", normalize, floor_us(4 * f_bytes, 0)), ("dist", dist, floor_us(2 * f_bytes + d_bytes, gemm)),
                         ("fwd", fwd, floor_us(d_bytes, 0)), ("bwd", bwd, floor_us(d_bytes + 3 * f_bytes, gemm))):
        t = time_events(fn, args.reps, args.warmup, args.burst)
        total += t[0]
        out.update({name + "_us_median_best_worst": t, name + "_floor_us": round(fl, 2), name + "_fraction_of_floor": round(fl / t[0], 3)})
    out.update({"sum_us_medians": round(total, 1), "L_mean": float(Lv.mean()), "m_min_max": [float(m.min()), float(m.max())]})
    print(json.dumps(out), flush=True)
    if args.step:
        gan_step_times(args, dev)


def gan_step_times(args, dev):
    """Trainer.gan_step of bench.py's networks with the term off and on: ms per step, median of --reps single replays of the captured
    step after --warmup replays; both twice, alternating (_loss_time.step_ab)."""
    out = {"what": f"Trainer.gan_step, 256 ch x 32 blocks, batch {args.batch}, {args.side // 4} -> {args.side}: ms per step [median, best, worst]"}
    out.update(step_ab([(f"alpha_cx_{alpha:g}", {"alpha_cx": alpha, "cx_h": args.h}) for alpha in (0.0, 1.0)], dev, args.batch, args.side,
                       args.reps, args.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
