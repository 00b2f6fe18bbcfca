"""What the four *_loss_time.py scripts share: the device-event timer, the floor of a kernel, and the A/B of a train step of the
full-size networks under sets of Trainer keyword arguments."""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS, MFMA_F32_TFLOPS = 6.29, 157.3


def time_events(fn, reps, warmup, calls=1, digits=2):
    """[median, best, worst] microseconds per call of `reps` bursts of `calls` back-to-back calls per device-event pair, after `warmup`
    calls; rounded to `digits` (None: as measured)."""
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
    out = [ts[len(ts) // 2], ts[0], ts[-1]]
    return out if digits is None else [round(v, digits) for v in out]


def floor_us(nbytes, flops):
    """The larger of bytes moved / 6.29 TB/s and issued FLOPs / 157.3 TFLOP/s, in microseconds."""
    return max(nbytes / HBM_TBS / 1e6, flops / MFMA_F32_TFLOPS / 1e6)


def step_ab(variants, dev, batch, side, reps, warmup, phase="train"):
    """A train step of bench.py's networks (256 channels x 32 blocks, LR side / 4 -> HR side) under every (key, Trainer keyword arguments)
    of `variants`, every variant twice, alternating: -> {key: {"ms": [median, best, worst], "logs": ...}, key + "_again": ...}.
    phase "train": gan_step, captured (the hipGraph of capture_gan_step, as bench.py runs it) after three eager steps, single replays;
    phase "pretrain": pretrain_step of the Generator alone, eager."""
    from model import VGG, Discriminator, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    gen = torch.Generator(device="cpu").manual_seed(7)
    hr = torch.randint(0, 256, (batch, 3, side, side), generator=gen).float().to(dev)
    lr = torch.nn.functional.avg_pool2d(hr, 4)
    out = {}
    for key, kw in tuple(variants) * 2:
        torch.manual_seed(0)
        opt = {"patch_size": side // 4, "num_channels": 256, "depth": 32, "res_scale": 0.1, "spectral_norm": False, "scale": 4}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            G = Generator(opt).to(dev)
            D, V = (Discriminator(opt).to(dev), VGG().to(dev)) if phase == "train" else (None, None)
        tr = Trainer(G, D, V, FlatAdam([p for p in G.parameters() if p.requires_grad], lr=1e-6),
                     FlatAdam(D.parameters(), lr=1e-6) if D is not None else None, **kw)
        run = tr.pretrain_step
        if phase == "train":
            for _ in range(3):                                            # first-use work must not happen under capture
                tr.gan_step(lr, hr)
            run = tr.capture_gan_step(lr, hr)
        logs = [None]

        def step():
            logs[0] = run(lr, hr)

        t = [round(v / 1e3, 3) for v in time_events(step, reps, warmup)]
        out[key + ("_again" if key in out else "")] = {"ms": t, "logs": {k: round(float(v), 6) for k, v in logs[0].items()}}
        del tr, G, D, V, run
        torch.cuda.empty_cache()
    return out
