"""Time of the texture loss's kernels (docs/modes.md section 4q) at the training shape: batch 16, HR 192 x 192, so the three VGG19 taps
are [16, 192, 192, 64], [16, 96, 96, 128] and [16, 48, 48, 256]; patches of 16 pixels a side and the whole map (patch 0).

  python scripts/texture_loss_time.py [--batch 16] [--side 192] [--patches 16,0] [--reps 21] [--warmup 3] [--burst 10] [--step]

Per tap and patch one JSON line: the C ABI calls pesr_gram_fwd (one feature tensor), pesr_gram_loss (with and without dG) and
pesr_gram_bwd, no allocation, in bursts of --burst back-to-back calls per device-event pair, divided by their number: median / best /
worst of --reps bursts after --warmup.  Beside each its FLOOR, the larger of bytes moved / 6.29 TB/s and issued FLOPs / 157.3 TFLOP/s,
and the fraction of the floor reached (floor / time).  Bytes: forward F read once and G written (with a split also the slabs written
and read); distance both G read, dG written; backward F and dG read, gF written.  Issued FLOPs: forward 2 K 1024 per computed 32 x 32
tile, C / 32 (C / 32 + 1) / 2 tiles per patch (only the upper triangle is computed; rows past an odd K are issued as zeros and not
counted); backward 2 K C C per patch.
--step: the captured Trainer.gan_step of the full-size networks (bench.py's: 256 channels x 32 blocks, batch 16, 48 -> 192) with the term off and on,
two trainers each, alternating: ms per step.  No pass/fail bar.
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
    ap.add_argument("--side", type=int, default=192, help="the HR side: the taps are side, side / 2, side / 4")
    ap.add_argument("--patches", type=str, default="16,0")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="also time Trainer.gan_step of the full-size networks with the term off and on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_loss_time.py measures on the GPU; none is visible")
    from pesr_amd import _lib, ops, texture
    dev = torch.device("cuda")
    L = _lib.lib()
    print(json.dumps({"library": _lib.LIB_PATH}), flush=True)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = args.batch
    for patch in (int(v) for v in args.patches.split(",")):
        total = {"fwd_sr_and_hr": 0.0, "loss": 0.0, "bwd": 0.0}
        for (h, w), c in zip(texture.tap_sizes(args.side, args.side), texture.TAP_CHANNELS):
            ph, pw = (patch or h), (patch or w)
            plan = ops.gram_plan(n, h, w, c, ph, pw)
            P, K, S = plan["patches"], plan["pixels"], plan["splits"]
            gen = torch.Generator(device="cpu").manual_seed(h * 10007 + c)
            fa = torch.randn((n, h, w, c), generator=gen).relu_().to(dev)
            fb = torch.randn((n, h, w, c), generator=gen).relu_().to(dev)
            Ga, Gb = ops.gram(fa, (ph, pw)), ops.gram(fb, (ph, pw))
            dg, gf = torch.empty_like(Ga), torch.empty_like(fa)
            t = torch.empty(n, dtype=torch.float64, device=dev)
            gout = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
            ws = ops.workspace(max(plan["workspace_bytes"], int(L.pesr_gram_loss_workspace_bytes(n, P, c))), dev)

            def fwd():
                _lib.check(L.pesr_gram_fwd(fa.data_ptr(), Ga.data_ptr(), n, h, w, c, ph, pw, ws.data_ptr(), ws.numel(), stream),
                           "pesr_gram_fwd")

            def loss(d=dg.data_ptr()):
                _lib.check(L.pesr_gram_loss(Ga.data_ptr(), Gb.data_ptr(), t.data_ptr(), d, n, P, c, ws.data_ptr(), ws.numel(), stream),
                           "pesr_gram_loss")

            def bwd():
                _lib.check(L.pesr_gram_bwd(fa.data_ptr(), dg.data_ptr(), gout.data_ptr(), gf.data_ptr(), n, h, w, c, ph, pw, stream),
                           "pesr_gram_bwd")

            t_fwd = time_events(fwd, args.reps, args.warmup, args.burst)
            t_loss = time_events(loss, args.reps, args.warmup, args.burst)
            t_value = time_events(lambda: loss(None), args.reps, args.warmup, args.burst)
            loss()
            t_bwd = time_events(bwd, args.reps, args.warmup, args.burst)
            f_bytes, g_bytes = fa.numel() * 4, Ga.numel() * 4
            tiles = (c // 32) * (c // 32 + 1) // 2
            fl_fwd = floor_us(f_bytes + g_bytes + (2 * S * g_bytes if S > 1 else 0), 2.0 * K * 1024 * tiles * n * P)
            fl_loss = floor_us(3 * g_bytes, 0)
            fl_bwd = floor_us(2 * f_bytes + g_bytes, 2.0 * K * c * c * n * P)
            total["fwd_sr_and_hr"] += 2 * t_fwd[0]
            total["loss"] += t_loss[0]
            total["bwd"] += t_bwd[0]
            print(json.dumps({"tap": [n, h, w, c], "patch": [ph, pw], "patches": P, "pixels": K, "splits": S,
                              "calls_per_event_pair": args.burst,
                              "fwd_us_median_best_worst": t_fwd, "fwd_floor_us": round(fl_fwd, 2), "fwd_fraction_of_floor": round(fl_fwd / t_fwd[0], 3),
                              "loss_with_dg_us_median_best_worst": t_loss, "loss_value_only_us_median_best_worst": t_value,
                              "loss_floor_us": round(fl_loss, 2), "loss_fraction_of_floor": round(fl_loss / t_loss[0], 3),
                              "bwd_us_median_best_worst": t_bwd, "bwd_floor_us": round(fl_bwd, 2), "bwd_fraction_of_floor": round(fl_bwd / t_bwd[0], 3),
                              "G_MB": round(g_bytes / 1e6, 2), "F_MB": round(f_bytes / 1e6, 2), "t_mean": float(t.mean())}), flush=True)
        print(json.dumps({"patch": patch, "us_per_step_three_taps_medians": {k: round(v, 1) for k, v in total.items()},
                          "sum_us": round(sum(total.values()), 1)}), flush=True)
    if args.step:
        gan_step_times(args, dev)


def gan_step_times(args, dev):
    """Trainer.gan_step of bench.py's networks with the term off, on with patches of 16 and on with the whole map: ms per step, median
    of --reps single replays of the captured step after --warmup replays; every variant twice, alternating (_loss_time.step_ab)."""
    out = {"what": f"Trainer.gan_step, 256 ch x 32 blocks, batch {args.batch}, {args.side // 4} -> {args.side}: ms per step [median, best, worst]"}
    out.update(step_ab([(f"alpha_texture_{alpha:g}" + (f"_patch_{patch}" if alpha else ""), {"alpha_texture": alpha, "texture_patch": patch})
                        for alpha, patch in ((0.0, 16), (1.0, 16), (1.0, 0))], dev, args.batch, args.side, args.reps, args.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
