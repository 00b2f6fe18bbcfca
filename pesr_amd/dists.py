"""DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity"), the texture-tolerant full-reference
perceptual score, as docs/modes.md section 4t restates it.

Two images in 0..255 go as ONE batch [a; b] through one per-channel affine (a MeanShift) and the VGG16 trunk that lpips.py builds (the
project's fp32 3x3 conv kernels with the fused ReLU), with every max-pool replaced by the L2 pooling of pesr_amd/csrc/dists.hip
(`ops.l2pool_fwd`).  Stage 0 is the image / 255 itself, stages 1 .. 5 the five taps of lpips.TAPS; at each stage the head kernel
(`ops.dists_layer`) takes the per-channel means, variances and covariance of both feature maps over the pixels, in float64, and sums
alpha_c S1_c + beta_c S2_c with the normalised weights.  The score is one minus the sum of the six stage sums, one float64 per image
pair.  There is no CPU path, and no loss term.

The project ships no weights.  `DistsModel.load(path)` reads the one file that

    python -m pesr_amd.dists pack --vgg16 VGG16_STATE_DICT --weights DISTS_WEIGHTS --out dists_vgg.pt

writes from a torchvision vgg16 state_dict and the published DISTS weights.pt (INTEGRATION.md says where a user gets the two);
`DistsModel.random(seed)` is for tests and smoke runs.
"""
from __future__ import annotations

import math
import os
import warnings

import torch
import torch.nn as nn

from . import ops
from .lpips import CFG, MIN_SIDE, TAP_CHANNELS, TORCHVISION_CONVS, _read_state_dict, conv_shapes, trunk_taps
from .model.basic import Conv, MeanShift, nchw, nhwc

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
STAGE_CHANNELS = (3,) + TAP_CHANNELS                                # the image, then relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
CHANNELS = sum(STAGE_CHANNELS)                                      # 1475
FORMAT = "pesr_amd.dists vgg16 v1"
assert CFG.count("M") == 4 and CHANNELS == 1475


class DistsModel(nn.Module):
    """The 13 conv weights and biases of the VGG16 trunk, alpha and beta (1475 each, float64) and the two input affines."""

    def __init__(self):
        super().__init__()
        with torch.random.fork_rng(devices=[]):                     # the constructors draw an initialisation: not from the caller's stream
            self.convs = nn.ModuleList(Conv(cin, cout, 3) for cout, cin in conv_shapes())
            # x = img / 255 (stage 0), and the trunk's input (x - mean) / std = img / (255 std) - mean / std
            self.unit = MeanShift(255.0, (0.0, 0.0, 0.0), (255.0, 255.0, 255.0))
            self.scaling = MeanShift(255.0, MEAN, tuple(255.0 * s for s in STD))
        self.register_buffer("alpha", torch.zeros(CHANNELS, dtype=torch.float64))
        self.register_buffer("beta", torch.zeros(CHANNELS, dtype=torch.float64))
        self._normalised = None
        for p in self.parameters():
            p.requires_grad = False

    # ---- construction ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def random(seed=0):
        """Kaiming-normal convs (torchvision's non-pretrained scheme) and alpha, beta ~ 0.1 + 0.01 N(0, 1), the published package's
        initialisation: the arithmetic of the metric with none of its meaning."""
        warnings.warn("pesr_amd DistsModel.random: no pretrained vgg16 / DISTS weights; random kaiming-normal features and random alpha, "
                      "beta (the VALUES are then not DISTS scores)")
        m = DistsModel()
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for conv in m.convs:
                std = (2.0 / (conv.out_channels * 9)) ** 0.5        # kaiming_normal_, fan_out, relu
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * std)
                conv.bias.zero_()
            m.alpha.copy_(0.1 + 0.01 * torch.randn(CHANNELS, generator=g, dtype=torch.float64))
            m.beta.copy_(0.1 + 0.01 * torch.randn(CHANNELS, generator=g, dtype=torch.float64))
        return m

    def tensors(self):
        """The file's content: {"format", "conv{i}.weight", "conv{i}.bias", "alpha", "beta"} as CPU tensors."""
        d = {"format": FORMAT}
        for i, conv in enumerate(self.convs):
            d[f"conv{i}.weight"] = conv.weight.detach().cpu().clone()
            d[f"conv{i}.bias"] = conv.bias.detach().cpu().clone()
        d["alpha"] = self.alpha.detach().cpu().clone()
        d["beta"] = self.beta.detach().cpu().clone()
        return d

    def save(self, path):
        torch.save(self.tensors(), path)

    @staticmethod
    def from_tensors(d, what):
        """A model from save()'s dictionary; ValueError naming the key that is missing, misshapen or non-finite, a sum(alpha) +
        sum(beta) that is not positive, or an LPIPS weight file."""
        from .lpips import FORMAT as LPIPS_FORMAT
        if isinstance(d, dict) and d.get("format") == LPIPS_FORMAT:
            raise ValueError(f"{what}: an LPIPS weight file (format {LPIPS_FORMAT!r}), not a DISTS one: pack one with `python -m "
                             "pesr_amd.dists pack`")
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError(f"{what}: not a DISTS weight file of `python -m pesr_amd.dists pack` (format {FORMAT!r})")
        m = DistsModel()

        def take(key, shape, dtype):
            t = d.get(key)
            if not torch.is_tensor(t):
                raise ValueError(f"{what}: {key}: missing")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{what}: {key}: shape {tuple(t.shape)}, expected {tuple(shape)}")
            t = t.detach().to(dtype)
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{what}: {key}: non-finite values")
            return t
        with torch.no_grad():
            for i, (conv, (cout, cin)) in enumerate(zip(m.convs, conv_shapes())):
                conv.weight.copy_(take(f"conv{i}.weight", (cout, cin, 3, 3), torch.float32))
                conv.bias.copy_(take(f"conv{i}.bias", (cout,), torch.float32))
            m.alpha.copy_(take("alpha", (CHANNELS,), torch.float64))
            m.beta.copy_(take("beta", (CHANNELS,), torch.float64))
        total = m.weight_sum()
        if not total > 0:
            raise ValueError(f"{what}: alpha, beta: sum(alpha) + sum(beta) = {total!r} is not positive (the score divides by it)")
        return m

    @staticmethod
    def load(path):
        """The file written by `pack` (or save()); ValueError with the reason otherwise.  No GPU is touched."""
        if not os.path.isfile(path):
            raise ValueError(f"{path}: no such file")
        try:
            d = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:
            raise ValueError(f"{path}: not readable as a DISTS weight file: {e}") from None
        return DistsModel.from_tensors(d, path)

    # ---- the weights -------------------------------------------------------------------------------------------------------------
    def weight_sum(self):
        """w = sum(alpha) + sum(beta) over all 1475 channels: math.fsum of the 2950 values, the exactly rounded sum (no order)."""
        return math.fsum(self.alpha.tolist() + self.beta.tolist())

    def normalised(self, device):
        """(alpha / w, beta / w) as float64 [1475] on `device`, each one IEEE division; computed once per device."""
        if self._normalised is None or self._normalised[0].device != device:
            w = self.weight_sum()
            self._normalised = ((self.alpha.cpu() / w).to(device), (self.beta.cpu() / w).to(device))
        return self._normalised

    # ---- the trunk ---------------------------------------------------------------------------------------------------------------
    def features(self, x):
        """[M, 3, H, W] images in 0..255, NCHW-contiguous -> the six NHWC stage tensors (the image / 255, then the five taps), always on
        the fp32 conv kernels; every pool is the L2 pooling."""
        with torch.no_grad():
            stage0 = nhwc(self.unit(x))
        return [stage0] + trunk_taps(self.scaling, self.convs, lambda h: nchw(ops.l2pool_fwd(nhwc(h))), x)


def load_model_flag(prog, flag, path):
    """Entry points: the model named by `flag`, or SystemExit naming the program and the flag.  No GPU is touched."""
    try:
        return DistsModel.load(path)
    except ValueError as e:
        raise SystemExit(f"{prog}: {flag} {e}")


def dists(a, b, model, shave=0, return_parts=False):
    """DISTS of N image pairs: float32 GPU tensors [N, 3, H, W] in 0..255, each in either memory format or a view; a border of `shave`
    pixels is dropped first -> device float64 [N]; with return_parts also the six per-stage sums [N] of alpha_c / w S1_c + beta_c / w
    S2_c (the score is one minus their sum in stage order).  ValueError if the shapes differ or the shaved image is smaller than
    16 x 16."""
    for t, name in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"dists: {name}: expected a [N, 3, H, W] float32 GPU tensor (there is no CPU path)")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"dists: the two images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    shave = int(shave)
    H, W = a.shape[2], a.shape[3]
    if shave < 0:
        raise ValueError(f"dists: shave must be >= 0, got {shave}")
    if H - 2 * shave < MIN_SIDE or W - 2 * shave < MIN_SIDE:
        raise ValueError(f"dists: a {H} x {W} image with shave {shave} leaves less than {MIN_SIDE} x {MIN_SIDE} (the rule of LPIPS, whose "
                         "trunk this is)")
    if model.alpha.device != a.device:
        model.to(a.device)
    aw, bw = model.normalised(a.device)
    with torch.no_grad():
        x = torch.cat([a.detach()[:, :, shave:H - shave, shave:W - shave], b.detach()[:, :, shave:H - shave, shave:W - shave]])
        x = x.contiguous()                                          # NCHW: the input affines fold the layout change
        total, parts, c0 = None, [], 0
        for f in model.features(x):
            c = f.shape[3]
            r = ops.dists_layer(f, aw[c0:c0 + c], bw[c0:c0 + c])
            c0 += c
            parts.append(r)
            total = r if total is None else total + r               # float64, stages in ascending order
        score = 1.0 - total
    return (score, parts) if return_parts else score


# ---- pack: the two published files -> the one file load() reads -----------------------------------------------------------------
def pack(vgg16_sd, weights_sd, what_vgg="--vgg16", what_weights="--weights"):
    """(torchvision vgg16 state_dict, the DISTS weights {"alpha", "beta"}) -> DistsModel; SystemExit names the offending key."""
    def take(d, what, key, shape):
        t = d.get(key)
        if not torch.is_tensor(t):
            raise SystemExit(f"dists pack: {what}: key {key} is missing")
        if shape is None:
            if t.numel() != CHANNELS:
                raise SystemExit(f"dists pack: {what}: key {key} has shape {tuple(t.shape)}, expected {CHANNELS} values")
        elif tuple(t.shape) != tuple(shape):
            raise SystemExit(f"dists pack: {what}: key {key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    d = {"format": FORMAT}
    for i, (idx, (cout, cin)) in enumerate(zip(TORCHVISION_CONVS, conv_shapes())):
        d[f"conv{i}.weight"] = take(vgg16_sd, what_vgg, f"features.{idx}.weight", (cout, cin, 3, 3))
        d[f"conv{i}.bias"] = take(vgg16_sd, what_vgg, f"features.{idx}.bias", (cout,))
    for key in ("alpha", "beta"):
        d[key] = take(weights_sd, what_weights, key, None).detach().reshape(CHANNELS).to(torch.float64)
    try:
        return DistsModel.from_tensors(d, "dists pack")
    except ValueError as e:
        raise SystemExit(str(e))


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m pesr_amd.dists", description="pack the DISTS weights into one file")
    sub = parser.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("pack")
    p.add_argument("--vgg16", required=True, help="a torchvision vgg16 state_dict (features.N.weight / .bias)")
    p.add_argument("--weights", required=True, help="the published DISTS weights.pt (alpha and beta, 1475 values each)")
    p.add_argument("--out", required=True, help="the file to write, for --dists / --valid_dists")
    args = parser.parse_args(argv)
    model = pack(_read_state_dict(args.vgg16, "--vgg16", "dists pack"), _read_state_dict(args.weights, "--weights", "dists pack"),
                 f"--vgg16 {args.vgg16}", f"--weights {args.weights}")
    model.save(args.out)
    print(f"{args.out}: VGG16 trunk ({len(model.convs)} convs), alpha and beta ({CHANNELS} each), DISTS")


if __name__ == "__main__":
    main()
