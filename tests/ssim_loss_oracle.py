"""CPU float64 restatement of SSIM-Y as a training loss (docs/modes.md section 4p), written from the definition and sharing no code
with pesr_amd.

The luma is NOT clipped and NOT rounded: Y = ((r*(65.738/256) + g*(129.057/256)) + b*(25.064/256)) + 16 in float64 from the float32
values.  Window, "valid" region, separable filtering (height pass, then width pass, acc = acc + g[k]*v for k ascending, product and sum
rounded separately - what numpy does for float64 arrays) and the map's expression order are those of section 4g.

score_ordered, coef_ordered and grad_ordered perform the device kernels' IEEE operations in the kernels' order (section 4p writes the
order down), the reduction tree of the score and the one rounding to float32 of the gradient included: the device results are compared
with them bit for bit.  grad_exact is torch.autograd on a float64 statement of the definition and knows nothing of that order.
"""
import numpy as np

from ssim_oracle import C1, C2, TAPS, _filter, window      # section 4g's window, constants and passes: one statement of them

HALO = TAPS - 1
KY = (65.738 / 256, 129.057 / 256, 25.064 / 256)
TILE_H, TILE_W, LANES, WAVE = 16, 32, 256, 64          # the forward's tile of the map and its workgroup: the score's summation order


def luma(img):
    """[3, H, W] floats -> float64 Y [H, W], neither clipped nor rounded."""
    rgb = np.asarray(img).astype(np.float64)
    return ((rgb[0] * KY[0] + rgb[1] * KY[1]) + rgb[2] * KY[2]) + 16.0


def _windows(a, b):
    """One pair [3, H, W] -> (S, ca, cb, cc), each [H-10, W-10]: the map and dS/dmx, dS/dxx, dS/dxy with the raw moments held fixed."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim != 3 or a.shape[0] != 3 or a.shape[1] < TAPS or a.shape[2] < TAPS:
        raise ValueError(f"ssim loss: two [3, H, W] images of equal size, sides >= {TAPS}, are required, got {a.shape} and {b.shape}")
    g = window()
    x, y = luma(a), luma(b)
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
    a1 = 2.0 * mxmy + C1
    a2 = 2.0 * sxy + C2
    b1 = (mxmx + mymy) + C1
    b2 = (sx + sy) + C2
    den = b1 * b2
    s = (a1 * a2) / den
    ca = ((2.0 * my) * (a2 - a1)) / den - ((2.0 * mx) * s) * (1.0 / b1 - 1.0 / b2)
    cb = -(s / b2)
    cc = (2.0 * a1) / den
    return s, ca, cb, cc


def map_ordered(a, b):
    """[N, 3, H, W] pairs -> the maps [N, H-10, W-10]."""
    return np.stack([_windows(p, q)[0] for p, q in zip(a, b)])


def coef_ordered(a, b):
    """[N, 3, H, W] pairs -> [N, 3, H-10, W-10]: ca, cb, cc of every window."""
    return np.stack([np.stack(_windows(p, q)[1:]) for p, q in zip(a, b)])


def _tree(v):
    """[..., 256] lane values -> [...]: within each wave of 64 lanes the butterfly v = v + v[lane ^ off], off = 32 .. 1, read at lane 0;
    then the four waves ((w0 + w1) + w2) + w3."""
    v = v.reshape(v.shape[:-1] + (LANES // WAVE, WAVE))
    lane = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _mean_ordered(s):
    """The device's mean of one map [Ho, Wo].  Per 16 x 32 tile: lane (row r, column pair c) = 16 r + c adds its two values in ascending
    x, then _tree.  The tiles' sums, row-major: lane t adds partials t, t + 256, ... ascending, then _tree; one division by Ho * Wo."""
    ho, wo = s.shape
    ty, tx = -(-ho // TILE_H), -(-wo // TILE_W)
    pad = np.zeros((ty * TILE_H, tx * TILE_W))
    pad[:ho, :wo] = s                                  # (a value outside the map is not added on the device; adding 0.0 is the same bits)
    t = pad.reshape(ty, TILE_H, tx, TILE_W // 2, 2).transpose(0, 2, 1, 3, 4)
    lanes = ((0.0 + t[..., 0]) + t[..., 1]).reshape(ty * tx, LANES)
    parts = _tree(lanes)
    rounds = -(-parts.size // LANES)
    p = np.zeros(rounds * LANES)
    p[:parts.size] = parts
    acc = np.zeros(LANES)
    for k in range(rounds):
        acc = acc + p[k * LANES:(k + 1) * LANES]
    return float(_tree(acc)) / (float(ho) * float(wo))


def score_ordered(a, b):
    """[N, 3, H, W] pairs -> float64 [N], bit for bit the device's score."""
    return np.array([_mean_ordered(_windows(p, q)[0]) for p, q in zip(a, b)])


def grad_ordered(a, b, gs, rounded=True):
    """d(sum_n gs[n] score[n]) / da in the device's order -> [N, 3, H, W], float32 (rounded once) or, with rounded=False, the float64
    values before that rounding.  The transpose of the valid filter is the full correlation with the window; the window is symmetric,
    so it is the valid filter of the map padded with 10 zeros on every side: the same passes, the same order."""
    g = window()
    out = []
    for p, q, gn in zip(np.asarray(a), np.asarray(b), np.asarray(gs, dtype=np.float64)):
        s, ca, cb, cc = _windows(p, q)
        ta, tb, tc = (_filter(np.pad(m, HALO), g) for m in (ca, cb, cc))
        x, y = luma(p), luma(q)
        u = (ta + (2.0 * x) * tb) + y * tc
        dy = (gn / (float(s.shape[0]) * float(s.shape[1]))) * u
        out.append(np.stack([dy * k for k in KY]))
    out = np.stack(out)
    return out.astype(np.float32) if rounded else out


def grad_exact(a, b, gs):
    """The same derivative by torch.autograd on the float64 definition (conv2d for the filters, any order of summation)."""
    import torch
    import torch.nn.functional as F
    g = torch.tensor(window(), dtype=torch.float64)
    ky = torch.tensor(KY, dtype=torch.float64).view(1, 3, 1, 1)
    ta = torch.from_numpy(np.array(a)).double().requires_grad_()
    tb = torch.from_numpy(np.array(b)).double()

    def filt(v):
        return F.conv2d(F.conv2d(v[:, None], g.view(1, 1, TAPS, 1)), g.view(1, 1, 1, TAPS))[:, 0]

    x, y = (ta * ky).sum(1) + 16.0, (tb * ky).sum(1) + 16.0
    mx, my = filt(x), filt(y)
    sx, sy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    smap = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    (smap.mean(dim=(1, 2)) * torch.from_numpy(np.array(gs, dtype=np.float64))).sum().backward()
    return ta.grad.numpy()
