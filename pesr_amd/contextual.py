"""Contextual loss (Mechrez et al.) of one VGG19 tap, as docs/modes.md section 4r defines it.

Every feature vector of the sr tap is matched to its nearest neighbour anywhere in the hr tap: with the P = H W points of both taps
centred on the hr mean and scaled to unit length, d_ij = (1 - xh_i . yh_j) / 2,

    w_ij = exp((1 - d_ij / (min_k d_ik + 1e-5)) / h),   c_ij = w_ij / sum_k w_ik,   CX = (1 / P) sum_j max_i c_ij,   L = -log CX.

The tap is relu3_4 (`features` index 17, 256 channels at a quarter of the HR resolution), out of the VGG19 trunk pass that the
perceptual loss runs anyway (`VGG.forward(sr, hr, taps=(17,))`); the two GEMMs and the reductions around them are the fp32 MFMA
kernels of pesr_amd/csrc/cx.hip (`ops.cx_normalize`, `ops.cx_dist`, `ops.cx_fwd`, `ops.cx_bwd`), whatever `ops.PRECISION` the convs
run in.
"""
from __future__ import annotations

from . import functional as PF

TAP = 17                                                            # relu3_4 of vgg19.features: the last ReLU in front of pool3
TAP_CHANNELS = 256
MAX_POINTS = 4096                                                   # the distance matrix is P x P per image


def tap_size(h: int, w: int):
    """The tap's (height, width) for an h x w image: two 2 x 2 max-pools lie in front of it."""
    return h >> 2, w >> 2


def check_size(h: int, w: int):
    """None if the contextual loss takes h x w images, else the reason.  Needs no device."""
    h, w = int(h), int(w)
    if h < 4 or w < 4 or h % 4 or w % 4:
        return f"both sides of the {h} x {w} image must be multiples of 4: the tap lies behind two 2 x 2 max-pools"
    th, tw = tap_size(h, w)
    if th * tw > MAX_POINTS:
        return f"the {th} x {tw} tap has {th * tw} points, the kernels take at most {MAX_POINTS}"
    return None


def contextual_from_tap(tap_sr, tap_hr, h: float = 0.5):
    """The relu3_4 taps of both passes (NHWC) -> device float64 [N], -log CX per image, differentiable with respect to the sr tap only."""
    if tap_sr.dim() != 4 or tuple(tap_sr.shape) != tuple(tap_hr.shape):
        raise ValueError(f"contextual_from_tap: expected two NHWC taps of one shape, got {tuple(tap_sr.shape)} and {tuple(tap_hr.shape)}")
    return PF.contextual_layer(tap_sr, tap_hr.detach(), float(h))
