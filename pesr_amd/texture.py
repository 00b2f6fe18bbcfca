"""Texture (style) loss: the distance between Gram matrices of VGG19 features, as docs/modes.md section 4q defines it.

Gatys et al. and Johnson et al. take the Gram matrix of a whole feature map; EnhanceNet (Sajjadi et al.) takes it patch-wise, on
16 x 16 patches of conv1_1 / conv2_1 / conv3_1.  Both are here: `patch` pixels a side, counted in each tap's own pixels, or 0 for the
whole map.  For a tapped NHWC feature tensor F [N, H, W, C] and patches of K pixels, P of them per image,

    G[n, p] = F_p^T F_p / (C K),    t_l[n] = (1 / P) sum_p sum_cc' (Gsr - Ghr)^2,    T[n] = t_1 + t_2 + t_3

over the taps relu1_1, relu2_1, relu3_1 in ascending order with equal weights.  The taps come out of the VGG19 trunk pass that the
perceptual loss runs anyway (`VGG.forward(sr, hr, taps=True)`); the Gram matrices, their distance and the gradient are the fp32 MFMA
kernels of pesr_amd/csrc/gram.hip (`ops.gram`, `ops.gram_loss`, `ops.gram_bwd`), whatever `ops.PRECISION` the convs run in.
"""
from __future__ import annotations

from . import functional as PF
from .model.vgg import VGG

TAPS = VGG.TAPS                                                     # (1, 6, 11): relu1_1, relu2_1, relu3_1 of vgg19.features
TAP_CHANNELS = (64, 128, 256)


def tap_sizes(h: int, w: int):
    """The three taps' (height, width) for an h x w image: one 2 x 2 max-pool (floor) in front of each tap after the first."""
    return [(h >> l, w >> l) for l in range(len(TAPS))]


def check_patch(h: int, w: int, patch: int):
    """None if the texture loss takes h x w images with this patch, else the reason.  Needs no device.  The same number is used at
    every tap, so it must divide h, h / 2, h / 4 and likewise w (which must be whole: the max-pool backward takes even sides only);
    0, the whole map, always fits."""
    patch = int(patch)
    if patch < 0:
        return f"the patch must be >= 0 (0 = the whole map), got {patch}"
    if patch == 0:
        return None
    if h < 4 or w < 4 or h % 4 or w % 4:
        return f"both sides of the {h} x {w} image must be multiples of 4: the taps lie behind up to two 2 x 2 max-pools"
    sizes = tap_sizes(h, w)
    if any(th % patch or tw % patch for th, tw in sizes):
        return (f"a patch of {patch} does not divide the three tap sizes " + ", ".join(f"{th} x {tw}" for th, tw in sizes))
    return None


def texture_from_taps(taps_sr, taps_hr, patch: int):
    """The three taps of both passes (NHWC, `VGG.forward(..., taps=True)`) -> device float64 [N], differentiable with respect to the
    sr taps only."""
    if len(taps_sr) != len(TAPS) or len(taps_hr) != len(TAPS):
        raise ValueError(f"texture_from_taps: expected {len(TAPS)} taps of each pass, got {len(taps_sr)} and {len(taps_hr)}")
    total = None
    for fa, fb in zip(taps_sr, taps_hr):
        t = PF.texture_layer(fa, fb.detach(), int(patch))
        total = t if total is None else total + t                   # float64, layers in ascending order
    return total
