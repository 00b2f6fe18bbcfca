"""Tiled inference (docs/modes.md section 4h) against the whole-image path, on the GPU.

  python scripts/tile_time.py time   [--sizes 339x510,128x128,64x64] [--pairs 32:8,80:8,64:16,56:68] [--reps 5] [--warmup 1]
  python scripts/tile_time.py approx [--size 339x510] [--core 56] [--halos 4,8,12,16,24,68]
  python scripts/tile_time.py kernels [--calls 200]

time: the full-size Generator (256 channels, 32 blocks, x4, seeded default-initialised weights) on one LR image per size - today's
path (`G(img)` and test.py's `x8_forward`) and `pesr_amd.tile.tiled_forward` at each (core:halo), plain and x8, alternating in one
process; device events around each call, every shape warmed up first; median / best / worst in ms, the number of tiles, computed
over image pixels, and the conv kernel families that ran (ops.FLOPS, algorithmic flops per family).  One JSON line per row.
approx: largest difference in grey levels and PSNR of the tiled uint8 result against the whole-image one as a function of the halo.
The weights are random - this shows how the error falls with the halo, not what a trained model gives.
kernels: --calls launches of pesr_tile_gather and pesr_tile_scatter on a 339 x 510 image (48 x 48 tiles, x8 members, x4), for
`rocprofv3 --kernel-trace --stats -- python scripts/tile_time.py kernels`; prints the bytes each launch moves.
No pass/fail bar.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS = 6.29


def stats(fn, reps, warmup):
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
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"ms_median": round(ts[len(ts) // 2], 3), "ms_best": round(ts[0], 3), "ms_worst": round(ts[-1], 3)}


def families(fn):
    from pesr_amd import ops
    ops.FLOPS.start()
    fn()
    torch.cuda.synchronize()
    by = ops.FLOPS.stop()["by_kernel_family"]
    return {k: round(v[0] / 1e9, 1) for k, v in by.items()}


def generator(dev):
    from model import Generator
    torch.manual_seed(0)
    return Generator({"num_channels": 256, "depth": 32, "res_scale": 0.1, "scale": 4}).to(dev).eval()


def image(h, w, dev):
    g = torch.Generator().manual_seed(h * 10007 + w)
    return torch.randint(0, 256, (1, 3, h, w), generator=g).float().to(dev)


def load_test_entry():
    import importlib.util
    spec = importlib.util.spec_from_file_location("entry_test", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    return T


def cmd_time(args, dev):
    from pesr_amd import tile
    T = load_test_entry()
    G = generator(dev)
    pairs = [tuple(int(v) for v in p.split(":")) for p in args.pairs.split(",")]
    with torch.no_grad():
        for size in args.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            img = image(h, w, dev)
            rows = [("whole image, G(img)", lambda: G(img), 1, 1.0), ("whole image, x8_forward", lambda: T.x8_forward(img, G), 1, 8.0)]
            for core, halo in pairs:
                th, tw, tiles = tile.plan(h, w, core, halo)
                ratio = len(tiles) * th * tw / (h * w)
                for ens in (False, True):
                    rows.append((f"tiled core {core} halo {halo}{', x8' if ens else ''}: {len(tiles)} tiles of {th} x {tw}",
                                 (lambda c=core, p=halo, e=ens: tile.tiled_forward(G, img, 4, c, p, args.batch, ensemble=e)), len(tiles),
                                 ratio * (8.0 if ens else 1.0)))
            fams = {what: families(fn) for what, fn, _, _ in rows}           # also the warm-up of every shape
            for rnd in range(args.rounds):                                     # alternating: every row once per round
                for what, fn, ntiles, ratio in rows:
                    r = {"what": what, "lr_image": [h, w], "round": rnd, "tiles": ntiles, "computed_over_image_pixels": round(ratio, 3),
                         "algorithmic_Gflop_by_conv_family": fams[what]}
                    r.update(stats(fn, args.reps, args.warmup))
                    print(json.dumps(r), flush=True)


def cmd_approx(args, dev):
    from pesr_amd import tile
    G = generator(dev)
    h, w = (int(v) for v in args.size.split("x"))
    img = image(h, w, dev)
    with torch.no_grad():
        whole = G(img)[0].clamp(0, 255).round()
        for halo in (int(v) for v in args.halos.split(",")):
            _, u8 = tile.tiled_forward(G, img, 4, args.core, halo, args.batch, f32=False, u8=True)
            d = (u8.permute(2, 0, 1).float() - whole).abs()
            mse = float((d * d).mean())
            th, tw, tiles = tile.plan(h, w, args.core, halo)
            print(json.dumps({"lr_image": [h, w], "core": args.core, "halo": halo, "tiles": len(tiles), "tile": [th, tw],
                              "max_grey_levels": int(d.max()), "differing_values_fraction": float((d > 0).float().mean()),
                              "psnr_db_vs_whole_image": (None if mse == 0 else round(10 * math.log10(255.0 ** 2 / mse), 2)),
                              "weights": "random (default init, seed 0): shows how the error falls with the halo only"}), flush=True)


def cmd_kernels(args, dev):
    from pesr_amd import ops, tile
    h, w, s = 339, 510, 4
    img = image(h, w, dev)[0].contiguous()
    u8 = img.permute(1, 2, 0).contiguous().to(torch.uint8)
    th, tw, tiles = tile.plan(h, w, 32, 8)
    desc8 = [(t[0], t[1], m) for t in tiles for m in range(8)]
    n = len(desc8)
    outs = torch.rand((n, 3, s * th, s * tw), device=dev) * 255.0
    p = torch.rand((len(tiles), 3, s * th, s * tw), device=dev) * 255.0
    of = torch.empty((3, s * h, s * w), device=dev)
    ou = torch.empty((s * h, s * w, 3), dtype=torch.uint8, device=dev)
    for _ in range(args.calls):
        ops.tile_gather(img, desc8, th, tw)
        ops.tile_gather(u8, desc8, th, tw)
        ops.tile_scatter(outs, None, tiles, 8, th, tw, s, h, w, of, ou, p, 0.6, 0.4)
        ops.tile_scatter(outs[:len(tiles)], None, tiles, 1, th, tw, s, h, w, of, None)
    torch.cuda.synchronize()
    owned = s * s * h * w
    gb = n * 3 * th * tw * 4
    print(json.dumps({"calls_of_each": args.calls, "tiles": len(tiles), "tile": [th, tw],
                      "gather_fp32_bytes": 2 * gb, "gather_u8_bytes": gb + gb // 4,
                      "scatter_E8_blend_both_outputs_bytes": owned * 3 * (8 * 4 + 4 + 4 + 1), "scatter_E1_fp32_bytes": owned * 3 * 8,
                      "us_at_6.29TBs": {"gather_fp32": round(2 * gb / HBM_TBS / 1e6, 2), "gather_u8": round((gb + gb // 4) / HBM_TBS / 1e6, 2),
                                        "scatter_E8": round(owned * 3 * 41 / HBM_TBS / 1e6, 2), "scatter_E1": round(owned * 24 / HBM_TBS / 1e6, 2)}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "approx", "kernels"])
    ap.add_argument("--sizes", default="339x510,128x128,64x64")
    ap.add_argument("--pairs", default="32:8,80:8,64:16,56:68")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--size", default="339x510")
    ap.add_argument("--core", type=int, default=56)
    ap.add_argument("--halos", default="4,8,12,16,24,68")
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_time.py measures on the GPU; none is visible")
    {"time": cmd_time, "approx": cmd_approx, "kernels": cmd_kernels}[args.mode](args, torch.device("cuda"))


if __name__ == "__main__":
    main()
