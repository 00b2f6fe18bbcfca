"""CPU float64 restatement of the bicubic resize of docs/modes.md section 4f (MATLAB's imresize for uint8 images and an integer
factor s in {2, 3, 4}, down and up), written from the definition and sharing no code with pesr_amd/resize.py.

One pass along one axis:  acc = 0; for taps ascending: acc = acc + w[t] * v[t]  (product and sum rounded separately, as numpy
does for float64 arrays), then floor(clip(acc, 0, 255) + 0.5).  Height first, then width, the intermediate image rounded to
uint8.  `rounded=False` skips both roundings (float64 out): the form that is compared with torch's antialiased bicubic.
"""
import numpy as np


def cubic(x):
    """Keys kernel, a = -0.5."""
    ax = abs(x)
    ax2 = ax * ax
    ax3 = ax2 * ax                     # plain products, left-to-right sums: the evaluation order is part of the definition
    if ax <= 1.0:
        return 1.5 * ax3 - 2.5 * ax2 + 1.0
    if ax <= 2.0:
        return -0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0
    return 0.0


def _normalised(raw):
    total = 0.0
    for v in raw:                      # ascending tap order
        total = total + v
    return [v / total for v in raw]


def down_taps(s):
    """-> (offsets t, weights): input index s*o + t, weight k((2t - (s-1)) / (2s)) / sum.  The two zero weights at x3 are kept."""
    offs = [t for t in range(-3 * s, 3 * s + 1) if abs(2 * t - (s - 1)) < 4 * s]
    return offs, _normalised([cubic((2 * t - (s - 1)) / (2 * s)) for t in offs])


def up_taps(s, p):
    """Phase p of the up-resize: output s*q + p reads inputs q + d ... q + d + 3 -> (d, weights)."""
    num = 2 * p + 1 - s                                   # c = q + num / (2s)
    d = (-1 if num < 0 else 0) - 1                        # floor(c) - 1 - q
    return d, _normalised([cubic((2 * s * (d + i) - num) / (2 * s)) for i in range(4)])


def weights(s, up):
    """The weight table in the layout of pesr_amd.resize.resize_weights: [taps] (down) or [s][4] (up)."""
    if up:
        return np.array([up_taps(s, p)[1] for p in range(s)], dtype=np.float64)
    return np.array(down_taps(s)[1], dtype=np.float64)


def reflect(j, n):
    """... 1 0 | 0 1 ... n-1 | n-1 n-2 ...  (period 2n)."""
    m = j % (2 * n)
    return m if m < n else 2 * n - 1 - m


def _finish(acc, rounded):
    return np.floor(np.clip(acc, 0, 255) + 0.5) if rounded else acc


def resize_axis0(a, s, up, rounded=True):
    """a: float64 array [n, ...] -> [n/s or s*n, ...] along axis 0."""
    n = a.shape[0]
    if up:
        out = np.empty((s * n,) + a.shape[1:], dtype=np.float64)
        for p in range(s):
            d, w = up_taps(s, p)
            for q in range(n):
                acc = np.zeros(a.shape[1:], dtype=np.float64)
                for i in range(4):
                    acc = acc + w[i] * a[reflect(q + d + i, n)]
                out[s * q + p] = _finish(acc, rounded)
        return out
    assert n % s == 0, (n, s)
    offs, w = down_taps(s)
    out = np.empty((n // s,) + a.shape[1:], dtype=np.float64)
    for o in range(n // s):
        acc = np.zeros(a.shape[1:], dtype=np.float64)
        for t, wt in zip(offs, w):
            acc = acc + wt * a[reflect(s * o + t, n)]
        out[o] = _finish(acc, rounded)
    return out


def imresize(img, s, up=False, rounded=True):
    """img: uint8 HWC -> uint8 HWC (rounded) or float64 HWC (rounded=False).  Height pass, then width pass."""
    assert s in (2, 3, 4)
    a = np.asarray(img).astype(np.float64)
    a = resize_axis0(a, s, up, rounded)
    a = resize_axis0(a.transpose(1, 0, 2), s, up, rounded).transpose(1, 0, 2)
    return np.ascontiguousarray(a.astype(np.uint8) if rounded else a)


def modcrop(img, s):
    return img[:img.shape[0] - img.shape[0] % s, :img.shape[1] - img.shape[1] % s]


def near_ties(img, s, up=False, eps=1e-9):
    """Diagnostic: how many pre-rounding values (both passes) lie within eps of a half-integer WITHOUT being one."""
    a = np.asarray(img).astype(np.float64)
    count = 0
    v = resize_axis0(a, s, up, rounded=False)
    f = np.abs(v - np.floor(v) - 0.5)
    count += int(((f < eps) & (f != 0)).sum())
    mid = np.floor(np.clip(v, 0, 255) + 0.5)
    v = resize_axis0(mid.transpose(1, 0, 2), s, up, rounded=False)
    f = np.abs(v - np.floor(v) - 0.5)
    count += int(((f < eps) & (f != 0)).sum())
    return count
