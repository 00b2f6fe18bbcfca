#!/usr/bin/env python3
"""Times of the U-Net discriminator (docs/modes.md section 4v) at the training shapes of batch 16, 192 x 192, d_width 64.

    python scripts/unet_d_time.py kernels     every new kernel: device-event median / best / worst of single launches, rotating through
                                              four sets of tensors so that no launch finds its input in the caches; for the streaming
                                              kernels the bytes the algorithm needs, GB/s and the share of 6.29 TB/s
    python scripts/unet_d_time.py modules     forward and forward + backward of D(x) alone, both discriminators, alternating
    python scripts/unet_d_time.py steps       the captured GAN step of the full-size Generator with --d_arch vgg / unet, alternating
    python scripts/unet_d_time.py bytes       the byte counts alone (no device)

Method as in docs/experiments/channel_attention.md: device events around each launch, medians with best and worst, A and B alternating in
one process."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.29e12
B, S, W0 = 16, 192, 64
UP_SHAPES = [(B, S // 8, S // 8, 8 * W0), (B, S // 4, S // 4, 4 * W0), (B, S // 2, S // 2, 2 * W0)]      # inputs of the three up2 calls


def up_bytes(shape, addends=1, backward=False):
    n = 4 * shape[0] * shape[1] * shape[2] * shape[3]
    return n * (4 + 1) if backward else n * (addends + 4)


def _stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def _time(fn, sets, reps=24):
    import torch
    for s in sets:
        fn(*s)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*sets[i % len(sets)]); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def _row(name, st, nbytes=None):
    med, lo, hi = (1e3 * v for v in st)
    tail = "" if nbytes is None else f"  {nbytes / 1e6:8.1f} MB  {nbytes / (med * 1e-6) / 1e9:7.0f} GB/s  {100 * nbytes / (med * 1e-6) / HBM:5.1f} % of 6.29 TB/s"
    print(f"{name:44s} {med:9.1f} us  (best {lo:9.1f}, worst {hi:9.1f}){tail}", flush=True)


def kernels():
    import torch
    from pesr_amd import ops
    r = lambda *s: torch.randn(*s, device="cuda")
    for shape in UP_SHAPES:
        sets = [(r(*shape), r(*shape)) for _ in range(4)]
        up = (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
        _row(f"up2 fwd {shape}", _time(lambda a, b: ops.bilinear_up2_fwd(a), sets), up_bytes(shape))
        _row(f"up2 fwd {shape} + addend", _time(ops.bilinear_up2_fwd, sets), up_bytes(shape, 2))
        del sets
        gsets = [(r(*up),) for _ in range(4)]
        _row(f"up2 bwd -> {shape}", _time(ops.bilinear_up2_bwd, gsets), up_bytes(shape, backward=True))
        del gsets
    n = B * S * S
    sets = [(r(B, 1, S, S), r(B, 1, S, S)) for _ in range(4)]
    for gan in ("SGAN", "RSGAN", "RaSGAN"):
        for side, focal in ((0, False), (1, True)):
            _row(f"gan_loss_map {gan} side {side} n={n}", _time(lambda a, b: ops.gan_loss_map(a, b, gan, side, focal, 1.0), sets))
    x = [(r(B, S, S, W0), r(1, W0, 3, 3), r(1), r(B, S, S, 1)) for _ in range(4)]
    xb = 4 * B * S * S * W0
    _row("conv9 fwd   [16,192,192,64] -> 1", _time(lambda a, w, b, g: ops.conv3x3_c1_fwd(a, w, b), x), xb + 4 * n)
    _row("conv9 dgrad [16,192,192,64] <- 1", _time(lambda a, w, b, g: ops.conv3x3_c1_dgrad(g, w, a.shape), x), xb + 4 * n)
    _row("conv9 wgrad [16,192,192,64] x 1", _time(lambda a, w, b, g: ops.conv3x3_c1_wgrad(a, g), x), xb + 4 * n)
    # the routed 3 x 3 path takes the forward (Cout padded to 16) and refuses both gradients: its forward, for the record
    wp = ops.pack_conv3x3(x[0][1], 0)
    _row("conv9 fwd on the padded implicit-GEMM path", _time(lambda a, w, b, g: ops.conv3x3_fwd(a, wp, b, 1), x), xb + 4 * n)


def _discriminators():
    import torch
    from pesr_amd.model import build_discriminator
    torch.manual_seed(0)
    opt = {"patch_size": S // 4, "spectral_norm": True, "scale": 4}
    return {"vgg": build_discriminator(opt).cuda(), "unet": build_discriminator(dict(opt, d_width=W0), "unet").cuda()}


def modules():
    import torch
    Ds = _discriminators()
    x = torch.rand(B, 3, S, S, device="cuda") * 255

    def fwd(D):
        with torch.no_grad():
            D(x)

    def both(D):
        for p in D.parameters():
            p.grad = None
        D(x).sum().backward()
    for _ in range(2):
        for name, D in Ds.items():
            _row(f"D {name} forward", _time(fwd, [(D,)], 12))
            _row(f"D {name} forward + backward", _time(both, [(D,)], 12))


def steps():
    import torch
    from model import VGG, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    torch.manual_seed(0)
    V = VGG().cuda()
    lr, hr = torch.rand(B, 3, S // 4, S // 4, device="cuda") * 255, torch.rand(B, 3, S, S, device="cuda") * 255
    runs = {}
    for name, D in _discriminators().items():
        G = Generator({"num_channels": 256, "depth": 32, "res_scale": 0.1, "scale": 4}).cuda()
        tr = Trainer(G, D, V, FlatAdam(G.parameters(), lr=5e-5), FlatAdam(D.parameters(), lr=5e-5))
        for _ in range(2):
            tr.gan_step(lr, hr)
        runs[name] = tr.capture_gan_step(lr, hr)
        print(f"D {name}: {sum(p.numel() for p in D.parameters()) / 1e6:.2f} M parameters", flush=True)
    for _ in range(3):
        for name, step in runs.items():
            _row(f"captured GAN step, --d_arch {name}", _time(lambda: step(lr, hr), [()], 10))


def bytes_():
    for shape in UP_SHAPES:
        print(f"up2 {shape}: forward {up_bytes(shape) / 1e6:.1f} MB, with the addend {up_bytes(shape, 2) / 1e6:.1f} MB, backward "
              f"{up_bytes(shape, backward=True) / 1e6:.1f} MB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "modules", "steps", "bytes"])
    {"kernels": kernels, "modules": modules, "steps": steps, "bytes": bytes_}[ap.parse_args().what]()
