"""LPIPS (Zhang et al., "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric", version 0.1, VGG variant), the
full-reference perceptual score, as docs/modes.md section 4n restates it.

Two images in 0..255 go through one per-channel affine (a MeanShift), the VGG16 trunk (the project's fp32 3x3 conv kernels with the
fused ReLU, the 2x2 max-pool) as ONE batch [a; b], and at each of the five taps the head kernel of pesr_amd/csrc/lpips.hip
(`ops.lpips_layer`): unit-normalise both feature vectors of a pixel, weighted squared difference, mean over the pixels.  The score
is the sum of the five layer scores, one float64 per image pair.  There is no CPU path.

The project ships no weights.  `LpipsModel.load(path)` reads the one file that

    python -m pesr_amd.lpips pack --vgg16 VGG16_STATE_DICT --lin LPIPS_LIN_STATE_DICT --out lpips_vgg.pt

writes from a torchvision vgg16 state_dict and the LPIPS v0.1 linear-layer file (INTEGRATION.md says where a user gets the two);
`LpipsModel.random(seed)` is for tests and smoke runs.

`lpips_loss(sr, hr, model)` is the same score as a training loss (docs/modes.md section 4o), differentiable with respect to sr: two
trunk passes (sr under autograd, hr under no_grad), the head's gradient kernel (`ops.lpips_layer_bwd`) at each tap, the trunk's input
gradients on the fp32 conv kernels whatever `ops.PRECISION` is when the backward runs.
"""
from __future__ import annotations

import os
import warnings

import torch
import torch.nn as nn

from . import functional as PF
from . import ops
from .model.basic import Conv, MeanShift, nhwc
from .model.vgg import _MaxPool

# VGG16 ("D") through conv5_3; a tap is the output after the ReLU of the conv at that index of the conv list
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)                                             # conv1_2, conv2_2, conv3_3, conv4_3, conv5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIDE = 16                                                       # four floor-mode pools must leave one pixel
FORMAT = "pesr_amd.lpips vgg16 v0.1"
# torchvision's vgg16.features indices of the 13 convs, and the LPIPS v0.1 file's keys of the five 1x1 layers
TORCHVISION_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
LIN_KEYS = tuple(f"lin{l}.model.1.weight" for l in range(5))


def conv_shapes():
    """[(Cout, Cin)] of the 13 convs."""
    out, c = [], 3
    for v in CFG:
        if v != "M":
            out.append((v, c))
            c = v
    return out


def trunk_taps(scaling, convs, pool, x):
    """The VGG16 trunk of CFG, shared with dists.py: [M, 3, H, W] images in 0..255 through the input affine `scaling`, the 13 `convs`
    with the fused ReLU and `pool` at every "M" -> the five tapped NHWC feature tensors, always on the fp32 conv kernels."""
    prev = ops.PRECISION
    ops.set_precision("fp32")                                       # the metric does not depend on the mode the generator runs in
    try:
        with torch.no_grad():
            h = scaling(x)
            taps, i = [], 0
            for v in CFG:
                if v == "M":
                    h = pool(h)
                    continue
                h = convs[i](h, act=ops.ACT_RELU)
                if i in TAPS:
                    taps.append(nhwc(h))
                i += 1
    finally:
        ops.set_precision(prev)
    return taps


class LpipsModel(nn.Module):
    """The 13 conv weights and biases of the VGG16 trunk, the five non-negative "lin" weight vectors, and the input affine."""

    def __init__(self):
        super().__init__()
        with torch.random.fork_rng(devices=[]):                     # the constructors draw an initialisation: not from the caller's stream
            self.convs = nn.ModuleList(Conv(cin, cout, 3) for cout, cin in conv_shapes())
            # x = img / 127.5 - 1, then (x - shift) / scale: img / (127.5 scale) - 127.5 (1 + shift) / (127.5 scale)
            self.scaling = MeanShift(127.5, tuple(1.0 + s for s in SHIFT), tuple(127.5 * s for s in SCALE))
        self.lins = nn.ParameterList(nn.Parameter(torch.zeros(c)) for c in TAP_CHANNELS)
        self.pool = _MaxPool()
        for p in self.parameters():
            p.requires_grad = False

    # ---- construction ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def random(seed=0):
        """Kaiming-normal convs (torchvision's non-pretrained scheme) and non-negative lin weights: the arithmetic of the metric with
        none of its meaning."""
        warnings.warn("pesr_amd LpipsModel.random: no pretrained vgg16 / LPIPS weights; random kaiming-normal features and random "
                      "non-negative linear layers (the VALUES are then not LPIPS scores)")
        m = LpipsModel()
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for conv in m.convs:
                std = (2.0 / (conv.out_channels * 9)) ** 0.5        # kaiming_normal_, fan_out, relu
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * std)
                conv.bias.zero_()
            for w in m.lins:
                w.copy_(torch.rand(w.shape, generator=g))
        return m

    def tensors(self):
        """The file's content: {"format", "conv{i}.weight", "conv{i}.bias", "lin{l}"} as CPU tensors."""
        d = {"format": FORMAT}
        for i, conv in enumerate(self.convs):
            d[f"conv{i}.weight"] = conv.weight.detach().cpu().clone()
            d[f"conv{i}.bias"] = conv.bias.detach().cpu().clone()
        for l, w in enumerate(self.lins):
            d[f"lin{l}"] = w.detach().cpu().clone()
        return d

    def save(self, path):
        torch.save(self.tensors(), path)

    @staticmethod
    def from_tensors(d, what):
        """A model from save()'s dictionary; ValueError naming the key that is missing, misshapen, non-finite or (lin) negative."""
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise ValueError(f"{what}: not an LPIPS weight file of `python -m pesr_amd.lpips pack` (format {FORMAT!r})")
        m = LpipsModel()

        def take(key, shape):
            t = d.get(key)
            if not torch.is_tensor(t):
                raise ValueError(f"{what}: {key}: missing")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{what}: {key}: shape {tuple(t.shape)}, expected {tuple(shape)}")
            t = t.detach().to(torch.float32)
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{what}: {key}: non-finite values")
            return t
        with torch.no_grad():
            for i, (conv, (cout, cin)) in enumerate(zip(m.convs, conv_shapes())):
                conv.weight.copy_(take(f"conv{i}.weight", (cout, cin, 3, 3)))
                conv.bias.copy_(take(f"conv{i}.bias", (cout,)))
            for l, (w, c) in enumerate(zip(m.lins, TAP_CHANNELS)):
                t = take(f"lin{l}", (c,))
                if bool((t < 0).any()):
                    raise ValueError(f"{what}: lin{l}: negative weights (LPIPS's linear layers are non-negative)")
                w.copy_(t)
        return m

    @staticmethod
    def load(path):
        """The file written by `pack` (or save()); ValueError with the reason otherwise.  No GPU is touched."""
        if not os.path.isfile(path):
            raise ValueError(f"{path}: no such file")
        try:
            d = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:
            raise ValueError(f"{path}: not readable as an LPIPS weight file: {e}") from None
        return LpipsModel.from_tensors(d, path)

    # ---- the trunk ---------------------------------------------------------------------------------------------------------------
    def features(self, x):
        """[M, 3, H, W] images in 0..255 -> the five tapped NHWC feature tensors, always on the fp32 conv kernels."""
        return trunk_taps(self.scaling, self.convs, lambda h: self.pool(h, relu_in=True), x)


    def features_grad(self, x):
        """features() of one image batch as a differentiable graph, for lpips_loss: every conv node carries the fp32 mode (forward and
        backward, functional.Conv3x3Fn's `precision`), so the input gradients that run later, inside some loss.backward(), do not
        depend on the mode set then, and no other network's node is touched.  Each tap is consumed twice, by the head and by the next
        conv or pool: autograd adds the two gradients and the tap's own conv masks the sum by its ReLU (relu_grad_by_consumer = False,
        and its consumers do not mask); every other ReLU is masked by the one conv that consumes it, as in model/vgg.py."""
        h = self.scaling(x)
        taps, i, masked_by_consumer = [], 0, False
        for v in CFG:
            if v == "M":
                h = self.pool(h, relu_in=masked_by_consumer)
                masked_by_consumer = False
                continue
            tap = i in TAPS
            h = self.convs[i](h, act=ops.ACT_RELU, relu_in=masked_by_consumer, relu_grad_by_consumer=not tap, precision="fp32")
            masked_by_consumer = not tap
            if tap:
                taps.append(nhwc(h))
            i += 1
        return taps


def load_model_flag(prog, flag, path):
    """Entry points: the model named by `flag`, or SystemExit naming the program and the flag.  No GPU is touched."""
    try:
        return LpipsModel.load(path)
    except ValueError as e:
        raise SystemExit(f"{prog}: {flag} {e}")


def lpips(a, b, model, shave=0, return_maps=False):
    """LPIPS of N image pairs: float32 GPU tensors [N, 3, H, W] in 0..255, each in either memory format or a view; a border of
    `shave` pixels is dropped first -> device float64 [N]; with return_maps also the five [N, h_l, w_l] maps d_l(p).  ValueError
    if the shapes differ or the shaved image is smaller than 16 x 16."""
    for t, name in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"lpips: {name}: expected a [N, 3, H, W] float32 GPU tensor (there is no CPU path)")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"lpips: the two images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    shave = int(shave)
    H, W = a.shape[2], a.shape[3]
    if shave < 0:
        raise ValueError(f"lpips: shave must be >= 0, got {shave}")
    if H - 2 * shave < MIN_SIDE or W - 2 * shave < MIN_SIDE:
        raise ValueError(f"lpips: a {H} x {W} image with shave {shave} leaves less than {MIN_SIDE} x {MIN_SIDE} (four 2 x 2 pools must "
                         "leave a pixel)")
    if model.lins[0].device != a.device:
        model.to(a.device)
    with torch.no_grad():
        x = torch.cat([a.detach()[:, :, shave:H - shave, shave:W - shave], b.detach()[:, :, shave:H - shave, shave:W - shave]])
        x = x.contiguous()                                          # NCHW: the input affine folds the layout change
        total, maps = None, []
        for f, w in zip(model.features(x), model.lins):
            r = ops.lpips_layer(f, w, return_maps)
            if return_maps:
                r, m = r
                maps.append(m)
            total = r if total is None else total + r               # float64, layers in ascending order
    return (total, maps) if return_maps else total


LOSS_SIDE = 16                                                      # four 2 x 2 pools, each with an even-sided input


def check_loss_side(h, w):
    """None if lpips_loss takes an h x w image (after the shave), else the reason."""
    if h < LOSS_SIDE or w < LOSS_SIDE or h % LOSS_SIDE or w % LOSS_SIDE:
        return (f"both sides must be multiples of {LOSS_SIDE} (at least {LOSS_SIDE}): the trunk has four 2 x 2 max-pools and the max-pool "
                "backward takes even sides only")
    return None


def lpips_loss(sr, hr, model, shave=0):
    """LPIPS of N image pairs as a loss: float32 GPU tensors [N, 3, H, W] in 0..255 -> device float64 [N], differentiable with respect
    to sr.  sr is taken as it is (no clamp, no rounding); hr is detached.  The value is lpips(sr, hr)'s definition; the trunk runs
    twice, on sr under autograd and on hr under no_grad (a [sr; hr] batch under autograd would run every input gradient on twice the
    images).  ValueError unless both shaved sides are multiples of 16: the max-pool backward takes even sides only."""
    for t, name in ((sr, "sr"), (hr, "hr")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"lpips_loss: {name}: expected a [N, 3, H, W] float32 GPU tensor (there is no CPU path)")
    if tuple(sr.shape) != tuple(hr.shape):
        raise ValueError(f"lpips_loss: the two images differ in shape: {tuple(sr.shape)} and {tuple(hr.shape)}")
    shave = int(shave)
    H, W = sr.shape[2], sr.shape[3]
    if shave < 0:
        raise ValueError(f"lpips_loss: shave must be >= 0, got {shave}")
    why = check_loss_side(H - 2 * shave, W - 2 * shave)
    if why:                                                         # (the shape rule first: it needs no device to be checked)
        raise ValueError(f"lpips_loss: a {H} x {W} image with shave {shave} leaves {max(H - 2 * shave, 0)} x {max(W - 2 * shave, 0)}; {why}")
    if not sr.is_cuda or not hr.is_cuda:
        raise ValueError("lpips_loss: expected [N, 3, H, W] float32 GPU tensors (there is no CPU path)")
    if model.lins[0].device != sr.device:
        model.to(sr.device)
    a, b = sr, hr.detach()
    if shave:
        a, b = a[:, :, shave:H - shave, shave:W - shave], b[:, :, shave:H - shave, shave:W - shave]
    taps_a = model.features_grad(a)
    with torch.no_grad():
        taps_b = model.features_grad(b)
    total = None
    for fa, fb, w in zip(taps_a, taps_b, model.lins):
        r = PF.lpips_layer(fa, fb, w)
        total = r if total is None else total + r                   # float64, layers in ascending order
    return total


# ---- pack: the two published files -> the one file load() reads -----------------------------------------------------------------
def _read_state_dict(path, flag, prog="lpips pack"):
    if not os.path.isfile(path):
        raise SystemExit(f"{prog}: {flag} {path}: no such file")
    try:
        d = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise SystemExit(f"{prog}: {flag} {path}: not readable as a state_dict: {e}")
    if not isinstance(d, dict):
        raise SystemExit(f"{prog}: {flag} {path}: not a state_dict")
    return d


def pack(vgg16_sd, lin_sd, what_vgg="--vgg16", what_lin="--lin"):
    """(torchvision vgg16 state_dict, LPIPS v0.1 linear-layer state_dict) -> LpipsModel; SystemExit names the offending key."""
    def take(d, what, key, shape):
        t = d.get(key)
        if not torch.is_tensor(t):
            raise SystemExit(f"lpips pack: {what}: key {key} is missing")
        if tuple(t.shape) != tuple(shape):
            raise SystemExit(f"lpips pack: {what}: key {key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    d = {"format": FORMAT}
    for i, (idx, (cout, cin)) in enumerate(zip(TORCHVISION_CONVS, conv_shapes())):
        d[f"conv{i}.weight"] = take(vgg16_sd, what_vgg, f"features.{idx}.weight", (cout, cin, 3, 3))
        d[f"conv{i}.bias"] = take(vgg16_sd, what_vgg, f"features.{idx}.bias", (cout,))
    for l, (key, c) in enumerate(zip(LIN_KEYS, TAP_CHANNELS)):
        d[f"lin{l}"] = take(lin_sd, what_lin, key, (1, c, 1, 1)).reshape(c)
    try:
        return LpipsModel.from_tensors(d, "lpips pack")
    except ValueError as e:
        raise SystemExit(str(e))


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m pesr_amd.lpips", description="pack the LPIPS (VGG, v0.1) weights into one file")
    sub = parser.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("pack")
    p.add_argument("--vgg16", required=True, help="a torchvision vgg16 state_dict (features.N.weight / .bias)")
    p.add_argument("--lin", required=True, help="the LPIPS v0.1 linear layers of the VGG variant (linN.model.1.weight)")
    p.add_argument("--out", required=True, help="the file to write, for --lpips / --valid_lpips")
    args = parser.parse_args(argv)
    model = pack(_read_state_dict(args.vgg16, "--vgg16"), _read_state_dict(args.lin, "--lin"),
                 f"--vgg16 {args.vgg16}", f"--lin {args.lin}")
    model.save(args.out)
    print(f"{args.out}: VGG16 trunk ({len(model.convs)} convs) and {len(model.lins)} linear layers, LPIPS v0.1")


if __name__ == "__main__":
    main()
