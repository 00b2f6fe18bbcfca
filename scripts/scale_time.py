"""GAN step time at x2, x3 and x4 (docs/modes.md section 4e) and the standalone r = 3 PixelShuffle's HBM rate.

  python scripts/scale_time.py [--steps 10] [--warmup 3]

Full-size model (256 channels, 32 blocks), B = 16, seeded random VGG weights, the captured step (Trainer.capture_gan_step, as
bench.py's default run) after eager warm-up steps.  Two families of settings: LR 48 at every scale, and HR 192 (patch 96 / 64 / 48).
Then pesr_pixel_shuffle_r_fwd / _bwd at [16,48,48,2304] <-> [16,144,144,256]: microseconds and effective TB/s
(bytes read + written / time) against the MI355X's 6.29 TB/s.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_TBS = 6.29


def time_events(fn, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def gan_step_time(scale, ps, steps, warmup, dev):
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    torch.manual_seed(0)
    opt = {"patch_size": ps, "num_channels": 256, "depth": 32, "res_scale": 0.1, "spectral_norm": False, "scale": scale}
    G, D = Generator(opt).to(dev), Discriminator(opt).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V = VGG().to(dev)
    tr = Trainer(G, D, V, FlatAdam(G.parameters(), lr=5e-5), FlatAdam(D.parameters(), lr=5e-5))
    B = 16
    lr = torch.randint(0, 256, (B, 3, ps, ps), device=dev).float()
    hr = torch.randint(0, 256, (B, 3, scale * ps, scale * ps), device=dev).float()
    for _ in range(warmup):
        tr.gan_step(lr, hr)
    step = tr.capture_gan_step(lr, hr)
    for _ in range(2):
        step(lr, hr)
    med, best = time_events(lambda: step(lr, hr), steps)
    del tr, G, D, V, step
    torch.cuda.empty_cache()
    return {"what": "GAN step (captured)", "scale": scale, "patch": ps, "hr": scale * ps, "batch": B, "ms_median": round(med, 3),
            "ms_best": round(best, 3), "patches_per_s": round(B / med * 1e3, 2)}


def shuffle_time(dev, reps=50):
    from pesr_amd import ops
    x = torch.rand(16, 48, 48, 2304, device=dev)
    dy = torch.rand(16, 144, 144, 256, device=dev)
    nbytes = 2 * x.numel() * 4
    out = []
    for name, fn in (("fwd", lambda: ops.pixel_shuffle_r_fwd(x, 3)), ("bwd", lambda: ops.pixel_shuffle_r_bwd(dy, 3))):
        for _ in range(5):
            fn()
        med, best = time_events(fn, reps)
        tbs = nbytes / (med * 1e-3) / 1e12
        out.append({"what": f"pixel_shuffle_r {name} r=3", "shape": "[16,48,48,2304] <-> [16,144,144,256]", "us_median": round(med * 1e3, 1),
                    "us_best": round(best * 1e3, 1), "TB_per_s": round(tbs, 3), "fraction_of_6.29": round(tbs / HBM_TBS, 3)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda")
    for row in shuffle_time(dev):
        print(json.dumps(row), flush=True)
    for scale, ps in ((4, 48), (3, 48), (2, 48), (3, 64), (2, 96)):     # LR 48 at each scale; HR 192 (x4's is the first row)
        print(json.dumps(gan_step_time(scale, ps, args.steps, args.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
