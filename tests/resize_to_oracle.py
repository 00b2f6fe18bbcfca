"""CPU float64 restatement of the any-size resize of docs/modes.md section 4m, written from the definition and sharing no code with
pesr_amd/resize.py.

One axis, n_in -> n_out, M = max(n_in, n_out): output o reads every input j with, for N = (2j+1) n_out - (2o+1) n_in, |N| < 4M
(bicubic), |N| < 2M (bilinear) or -M <= N < M (box), in ascending j, at the kernel argument N / (2M) - one integer divided once; the
weights are divided by their sum taken in ascending order; the index is reflected symmetrically (period 2 n_in); acc = 0, then acc =
acc + w * v per tap (product and sum rounded separately, as numpy does for float64 arrays); the width pass may add sigma_n * g(q, e),
e = (y * w_out + x) * 3 + c (tests/degrade_oracle.py's g); floor(clip(acc, 0, 255) + 0.5).  Height pass, uint8, width pass.
"""
import numpy as np

import degrade_oracle as DO

METHODS = ("bicubic", "bilinear", "box")


def kernel(method, num, den):
    """h(num / den) of the filter."""
    x = abs(num) / den
    if method == "bicubic":
        x2 = x * x
        x3 = x2 * x
        if x <= 1.0:
            return 1.5 * x3 - 2.5 * x2 + 1.0
        if x <= 2.0:
            return -0.5 * x3 + 2.5 * x2 - 4.0 * x + 2.0
        return 0.0
    if method == "bilinear":
        return 1.0 - x if x <= 1.0 else 0.0
    assert method == "box", method
    return 1.0


def inside(method, N, M):
    if method == "bicubic":
        return abs(N) < 4 * M
    if method == "bilinear":
        return abs(N) < 2 * M
    return -M <= N < M


def taps(n_in, n_out, method):
    """-> per output o: (list of unreflected taps j, ascending and contiguous; list of normalised float64 weights)."""
    assert n_in >= 1 and n_out >= 1 and n_in <= 8 * n_out and n_out <= 8 * n_in and method in METHODS
    M = max(n_in, n_out)
    rows = []
    for o in range(n_out):
        centre = ((2 * o + 1) * n_in) // (2 * n_out)              # a point inside the support; the scan around it is generous
        js = [j for j in range(centre - 40, centre + 41) if inside(method, (2 * j + 1) * n_out - (2 * o + 1) * n_in, M)]
        assert js and js == list(range(js[0], js[-1] + 1)) and js[0] > centre - 40 and js[-1] < centre + 40
        raw = [kernel(method, (2 * j + 1) * n_out - (2 * o + 1) * n_in, 2 * M) for j in js]
        total = 0.0
        for v in raw:
            total = total + v
        rows.append((js, [v / total for v in raw]))
    return rows


def reflect(j, n):
    m = j % (2 * n)
    return m if m < n else 2 * n - 1 - m


def resize_axis0(a, n_out, method):
    """float64 [n_in, ...] -> float64 [n_out, ...], unrounded: sequential over the taps, vectorised over everything else."""
    n_in = a.shape[0]
    out = np.zeros((n_out,) + a.shape[1:], dtype=np.float64)
    for o, (js, ws) in enumerate(taps(n_in, n_out, method)):
        acc = np.zeros(a.shape[1:], dtype=np.float64)
        for j, w in zip(js, ws):
            acc = acc + w * a[reflect(j, n_in)]
        out[o] = acc
    return out


def _round(acc):
    return np.floor(np.clip(acc, 0, 255) + 0.5).astype(np.uint8)


def resize(img, size, method="bicubic", sigma_n=0.0, q=0, rounded=True):
    """img: uint8 HWC -> size = (h_out, w_out), uint8 HWC (rounded) or the float64 values of the width pass before the clamp and the
    rounding (rounded=False; the intermediate image is rounded either way)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    ho, wo = size
    mid = _round(resize_axis0(img.astype(np.float64), ho, method))
    acc = resize_axis0(mid.astype(np.float64).transpose(1, 0, 2), wo, method).transpose(1, 0, 2)
    if sigma_n != 0:
        acc = acc + sigma_n * DO.gauss(q, ho * wo * 3).reshape(ho, wo, 3)
    return _round(acc) if rounded else acc


def near_ties(img, size, method="bicubic", sigma_n=0.0, q=0, eps=1e-9):
    """Diagnostic: how many pre-rounding values of the width pass lie within eps of a half-integer WITHOUT being one."""
    v = resize(img, size, method, sigma_n, q, rounded=False)
    f = np.abs(v - np.floor(v) - 0.5)
    return int(((f < eps) & (f != 0)).sum())


def jitter_size(n, r):
    """Q(n) = min(8n, max(ceil(n / 8), floor(r n + 0.5)))."""
    return min(8 * n, max(-(-n // 8), int(np.floor(r * n + 0.5))))


def jitter(img, r, m1, m2, sigma_n=0.0, q=0):
    """The resize-jitter round trip: h x w -> Q(h) x Q(w) with filter m1, back to h x w with m2, the noise in the second resize."""
    h, w = img.shape[:2]
    return resize(resize(img, (jitter_size(h, r), jitter_size(w, r)), METHODS[m1]), (h, w), METHODS[m2], sigma_n, q)
