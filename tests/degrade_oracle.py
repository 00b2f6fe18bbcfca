"""CPU float64 restatement of the classical degradation of docs/modes.md section 4j, LR = (HR (*) k) subsampled by s, plus noise,
written from the definition and sharing no code with pesr_amd/degrade.py.

LR pixel (oy, ox) of an H x W image reads HR rows s*oy + (s-K)/2 + i, i = 0 .. K-1 (columns likewise with j), clamped to the image;
acc = 0; for i ascending, for j ascending: acc = acc + k[i][j] * v  (product and sum rounded separately, as numpy does for float64
arrays); element e = (y*w + x)*3 + c of the window gets acc = acc + sigma_n * g(q, e) unless sigma_n == 0; then
floor(clip(acc, 0, 255) + 0.5).  Vectorised over the pixels of the window, sequential over the taps.
"""
import math

import numpy as np

_M = (1 << 64) - 1


def splitmix64(z):
    """numpy uint64 array (or Python int) -> the same, one round of the mixer of oracle/detrand.py."""
    if isinstance(z, int):
        z = (z + 0x9E3779B97F4A7C15) & _M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
        return z ^ (z >> 31)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def gauss(q, n, first=0):
    """g(q, e) for e = first .. first + n - 1: float64 [n]."""
    key = np.uint64(splitmix64(int(q) & _M))
    e = np.arange(first, first + n, dtype=np.uint64)
    total = np.zeros(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(3):
            z = splitmix64(key + np.uint64(3) * e + np.uint64(j))
            for sh in (0, 16, 32, 48):
                total += ((z >> np.uint64(sh)) & np.uint64(0xffff)).astype(np.int64)
    return (2 * total - 786420).astype(np.float64) / 131072.0


def legal(s, K):
    return s in (2, 3, 4) and 1 <= K <= 24 and (K - s) % 2 == 0


def gaussian_kernel(K, sigma1, sigma2=None, theta=0.0):
    """[K][K] float64: exp(-0.5 (a u^2 + 2 b u v + c v^2)) with [[a, b], [b, c]] = R diag(1/sigma1^2, 1/sigma2^2) R^T, normalised by
    the row-major sequential sum."""
    sigma2 = sigma1 if sigma2 is None else sigma2
    ct, st = math.cos(theta), math.sin(theta)
    i1, i2 = 1.0 / (sigma1 * sigma1), 1.0 / (sigma2 * sigma2)
    a = ct * ct * i1 + st * st * i2
    b = ct * st * (i1 - i2)
    c = st * st * i1 + ct * ct * i2
    t = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    u, v = np.meshgrid(t, t)                       # u along columns, v along rows
    w = np.exp(-0.5 * (a * (u * u) + (2.0 * b) * (u * v) + c * (v * v)))
    total = 0.0
    for x in w.reshape(-1):
        total = total + x
    return w / total


def degrade(img, s, kernel, sigma_n=0.0, q=0, window=None, rounded=True):
    """img: uint8 HWC, sides multiples of s -> the window (y0, x0, h, w) of its LR image (None: all of it), uint8 HWC (rounded) or
    float64 HWC before the clamp and the rounding (rounded=False)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    k = np.asarray(kernel, dtype=np.float64)
    K = k.shape[0]
    assert k.shape == (K, K) and legal(s, K) and H % s == 0 and W % s == 0
    y0, x0, h, w = window if window is not None else (0, 0, H // s, W // s)
    assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H // s and x0 + w <= W // s
    a = img.astype(np.float64)
    first = (s - K) // 2                              # exact: s - K is even
    rows0 = s * (y0 + np.arange(h)) + first
    cols0 = s * (x0 + np.arange(w)) + first
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for i in range(K):
        r = np.clip(rows0 + i, 0, H - 1)
        for j in range(K):
            c = np.clip(cols0 + j, 0, W - 1)
            acc = acc + k[i, j] * a[r[:, None], c[None, :]]
    if sigma_n != 0:
        acc = acc + sigma_n * gauss(q, h * w * 3).reshape(h, w, 3)
    if not rounded:
        return acc
    return np.floor(np.clip(acc, 0, 255) + 0.5).astype(np.uint8)


def near_ties(img, s, kernel, sigma_n=0.0, q=0, window=None, eps=1e-9):
    """Diagnostic: how many pre-rounding values lie within eps of a half-integer WITHOUT being one."""
    v = degrade(img, s, kernel, sigma_n, q, window, rounded=False)
    f = np.abs(v - np.floor(v) - 0.5)
    return int(((f < eps) & (f != 0)).sum())


def modcrop(img, s):
    return img[:img.shape[0] - img.shape[0] % s, :img.shape[1] - img.shape[1] % s]
