"""CPU float64 restatement of the SSIM-Y of docs/modes.md section 4g: the SSIM of Wang et al.'s ssim_index.m as the super-resolution
literature uses it (Y channel, 11 x 11 Gaussian window of sigma 1.5, "valid" region, K1 = 0.01, K2 = 0.03, L = 255, an optional
border shave), written from the definition and sharing no code with utils.compute_SSIM or pesr_amd.

Luma is the one of the PSNR-Y (utils.compute_PSNR, psnr_y_kernel): RGB clipped to 0..255 and rounded to integers,
y = ((r * (65.738/256) + g * (129.057/256)) + b * (25.064/256)) + 16 in double, clipped and rounded again.  (The division by 256 is
a power of two, so this equals (65.738 r + 129.057 g + 25.064 b)/256 + 16 bit for bit.)

Filtering is separable: height pass, then width pass, each  acc = 0; for k ascending: acc = acc + g[k] * v  with the product and
the sum rounded separately (what numpy does for float64 arrays: no fused multiply-add).  The evaluation order of every expression
below is part of the definition: the device kernel reproduces every bit of the map.
"""
import math

import numpy as np

C1 = (0.01 * 255) * (0.01 * 255)
C2 = (0.03 * 255) * (0.03 * 255)
TAPS = 11


def window():
    """g[k] = exp(-(k-5)^2 / 4.5) / sum, the sum accumulated in ascending k."""
    raw = [math.exp(-((k - 5) * (k - 5)) / 4.5) for k in range(TAPS)]
    total = 0.0
    for v in raw:
        total = total + v
    return [v / total for v in raw]


def luma(img):
    """[3, H, W] array of 0..255 values (any floats) -> integer-valued float64 Y [H, W]."""
    rgb = np.rint(np.clip(np.asarray(img).astype(np.float64), 0.0, 255.0))
    y = ((rgb[0] * (65.738 / 256) + rgb[1] * (129.057 / 256)) + rgb[2] * (25.064 / 256)) + 16.0
    return np.rint(np.clip(y, 0.0, 255.0))


def _filter(v, g):
    """Separable "valid" filtering of [H, W]: along the height, then along the width."""
    ho = v.shape[0] - (TAPS - 1)
    wo = v.shape[1] - (TAPS - 1)
    acc = np.zeros((ho, v.shape[1]))
    for k in range(TAPS):
        acc = acc + g[k] * v[k:k + ho, :]
    out = np.zeros((ho, wo))
    for k in range(TAPS):
        out = out + g[k] * acc[:, k:k + wo]
    return out


def ssim_map_y(x, y):
    """SSIM map of two integer-valued float64 Y images [H, W] -> [H-10, W-10]."""
    if x.shape != y.shape or x.ndim != 2:
        raise ValueError(f"ssim: two Y images of equal size are required, got {x.shape} and {y.shape}")
    if x.shape[0] < TAPS or x.shape[1] < TAPS:
        raise ValueError(f"ssim: the image (after the shave) is {x.shape[0]} x {x.shape[1]}, below the {TAPS} x {TAPS} window")
    g = window()
    mx = _filter(x, g)
    my = _filter(y, g)
    xx = _filter(x * x, g)
    yy = _filter(y * y, g)
    xy = _filter(x * y, g)
    mxmx = mx * mx
    mymy = my * my
    mxmy = mx * my
    sx = xx - mxmx
    sy = yy - mymy
    sxy = xy - mxmy
    num = (2.0 * mxmy + C1) * (2.0 * sxy + C2)
    den = ((mxmx + mymy) + C1) * ((sx + sy) + C2)
    return num / den


def ssim_map(a, b, shave=0):
    """SSIM-Y map of two RGB images [3, H, W] (0..255 floats), a border of `shave` pixels ignored -> [H-2*shave-10, W-2*shave-10]."""
    a = np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"ssim: two [3, H, W] images of equal size are required, got {a.shape} and {b.shape}")
    if shave < 0:
        raise ValueError(f"ssim: shave must be >= 0, got {shave}")
    H, W = a.shape[1], a.shape[2]
    return ssim_map_y(luma(a)[shave:H - shave, shave:W - shave], luma(b)[shave:H - shave, shave:W - shave])


def ssim(a, b, shave=0):
    """Mean of the map, summed exactly (math.fsum) and divided once."""
    m = ssim_map(a, b, shave)
    return math.fsum(m.ravel().tolist()) / m.size
