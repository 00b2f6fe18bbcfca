"""CPU float64 restatement of the NIQE of docs/modes.md section 4k (Mittal et al.'s computequality.m, computefeature.m,
estimateaggdparam.m and estimatemodelparam.m), written from the definition and sharing no code with pesr_amd/niqe.py or utils.

Luma of the clipped and rounded RGB ("gray": MATLAB's rgb2gray; "y": the Y of the PSNR-Y), a border shave, a top-left crop to
multiples of the block side B; scale 2 is the x0.5 antialiased bicubic resize of the cropped luma (section 4f's taps and reflect
rule, height then width, nothing rounded or clamped).  Per scale the MSCN map; per block 26 sums, summed exactly (math.fsum); per
block 36 features from AGGD fits; the score against a model.  Filter passes are  acc = 0; acc = acc + g[k] * v  in ascending k,
product and sum rounded separately (what numpy does for float64 arrays).  The evaluation order of every expression is part of the
definition: the device kernel reproduces every bit of both MSCN maps.
"""
import math

import numpy as np

TAPS = 7
DOWN_W = [-3 / 256, -9 / 256, 29 / 256, 111 / 256, 111 / 256, 29 / 256, -9 / 256, -3 / 256]
SHIFTS = [(0, 1), (1, 0), (1, 1), (1, -1)]


def window():
    """g[k] = exp(-(k-3)^2 / (2 (7/6)^2)) / sum, the sum accumulated in ascending k."""
    s = 7 / 6
    raw = [math.exp(-((k - 3) * (k - 3)) / (2 * (s * s))) for k in range(TAPS)]
    total = 0.0
    for v in raw:
        total = total + v
    return [v / total for v in raw]


def luma(img, mode="gray"):
    """[3, H, W] of 0..255 values (any floats) -> integer-valued float64 [H, W]."""
    rgb = np.rint(np.clip(np.asarray(img).astype(np.float64), 0.0, 255.0))
    r, g, b = rgb[0], rgb[1], rgb[2]
    if mode == "gray":
        return np.floor(((r * 0.298936021293775 + g * 0.587043074451121) + b * 0.114020904255103) + 0.5)
    if mode == "y":
        y = ((r * (65.738 / 256) + g * (129.057 / 256)) + b * (25.064 / 256)) + 16.0
        return np.rint(np.clip(y, 0.0, 255.0))
    raise ValueError(f"niqe: unknown luma mode {mode!r}")


def crop(y, shave, B):
    if shave < 0:
        raise ValueError(f"niqe: shave must be >= 0, got {shave}")
    if B % 2 or B < 8 or B > 96:
        raise ValueError(f"niqe: B must be even and in 8..96, got {B}")
    H, W = y.shape[0] - 2 * shave, y.shape[1] - 2 * shave
    nby, nbx = max(H, 0) // B, max(W, 0) // B
    if nby * nbx < 2:
        raise ValueError(f"niqe: {nby * nbx} block(s) of {B}: a covariance needs two rows")
    return y[shave:shave + nby * B, shave:shave + nbx * B]


def reflect(j, n):
    m = j % (2 * n)
    return m if m < n else 2 * n - 1 - m


def down2_axis0(a):
    n = a.shape[0]
    out = np.empty((n // 2,) + a.shape[1:])
    for o in range(n // 2):
        acc = np.zeros(a.shape[1:])
        for t in range(8):
            acc = acc + DOWN_W[t] * a[reflect(2 * o - 3 + t, n)]
        out[o] = acc
    return out


def down2(a):
    return np.ascontiguousarray(down2_axis0(down2_axis0(a).T).T)


def filt(a):
    """Separable "same" filtering with replicated edges: along the height, then along the width."""
    g = window()
    H, W = a.shape
    rows = [min(max(i, 0), H - 1) for i in range(-3, H + 3)]
    acc = np.zeros((H, W))
    for k in range(TAPS):
        acc = acc + g[k] * a[rows[k:k + H], :]
    cols = [min(max(i, 0), W - 1) for i in range(-3, W + 3)]
    out = np.zeros((H, W))
    for k in range(TAPS):
        out = out + g[k] * acc[:, cols[k:k + W]]
    return out


def mscn(a):
    """-> (MSCN map, sigma map)."""
    mu = filt(a)
    sq = filt(a * a)
    mumu = mu * mu
    sigma = np.sqrt(np.abs(sq - mumu))
    return (a - mu) / (sigma + 1.0), sigma


def circshift(m, d):
    """MATLAB's circshift: out[i][j] = m[(i - d0) mod n0][(j - d1) mod n1]."""
    return np.roll(m, d, axis=(0, 1))


def five(x):
    """One map -> [sum x*x over x < 0, count x < 0, sum x*x over x > 0, count x > 0, sum |x|]."""
    v = x.ravel()
    neg, pos = v[v < 0], v[v > 0]
    return [math.fsum((neg * neg).tolist()), float(len(neg)), math.fsum((pos * pos).tolist()), float(len(pos)),
            math.fsum(np.abs(v).tolist())]


def block_stats(m, sigma, bs):
    """-> [nby*nbx][26]."""
    nby, nbx = m.shape[0] // bs, m.shape[1] // bs
    out = []
    for by in range(nby):
        for bx in range(nbx):
            blk = m[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs]
            row = five(blk)
            for d in SHIFTS:
                row += five(blk * circshift(blk, d))     # the shift wraps INSIDE the block
            row.append(math.fsum(sigma[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs].ravel().tolist()))
            out.append(row)
    return np.array(out)


def stats(img, shave=0, B=96, mode="gray"):
    """[3, H, W] -> (stats [2][nblk][26], MSCN map of scale 1, MSCN map of scale 2)."""
    i1 = crop(luma(img, mode), shave, B)
    m1, s1 = mscn(i1)
    m2, s2 = mscn(down2(i1))
    return np.stack([block_stats(m1, s1, B), block_stats(m2, s2, B // 2)]), m1, m2


_GRID = None


def grid():
    global _GRID
    if _GRID is None:
        a = [(200 + i) / 1000 for i in range(9801)]
        r = [math.gamma(2 / v) * math.gamma(2 / v) / (math.gamma(1 / v) * math.gamma(3 / v)) for v in a]
        _GRID = (a, np.array(r))
    return _GRID


def aggd(L2, nl, R2, nr, A, n):
    """-> (grid index, alpha, bl, br, rn, gap): gap is the difference between the best and the second-best grid distance |r(a) - rn|,
    relative to rn (how far rn is from the point where the choice of alpha flips).  None where a side is empty."""
    if nl == 0 or nr == 0:
        return None
    a, r = grid()
    ls = math.sqrt(L2 / nl)
    rs = math.sqrt(R2 / nr)
    gh = ls / rs
    rhat = ((A / n) * (A / n)) / ((L2 + R2) / n)
    gh2 = gh * gh
    rn = rhat * (gh2 * gh + 1.0) * (gh + 1.0) / ((gh2 + 1.0) * (gh2 + 1.0))
    if not math.isfinite(rn):
        return None
    d = r - rn
    i = int(np.argmin(d * d))                       # numpy's argmin returns the FIRST minimiser
    dist = np.sort(np.abs(d))
    gap = float(dist[1] - dist[0]) / rn
    al = a[i]
    c = math.sqrt(math.gamma(1 / al) / math.gamma(3 / al))
    return i, al, ls * c, rs * c, rn, gap


def features(st, B):
    """stats [2][nblk][26] -> (features [nblk][36] with NaN rows for dropped blocks, grid indices [nblk][10] (-1 where dropped), the
    smallest gap over all fits)."""
    nblk = st.shape[1]
    feat = np.full((nblk, 36), np.nan)
    index = np.full((nblk, 10), -1, dtype=np.int64)
    min_gap = math.inf
    for b in range(nblk):
        row, ok = [], True
        for sc in range(2):
            n = float((B >> sc) * (B >> sc))
            for q in range(5):
                fit = aggd(*[float(v) for v in st[sc, b, 5 * q:5 * q + 5]], n)
                if fit is None:
                    ok = False
                    continue
                i, al, bl, br, rn, gap = fit
                index[b, 5 * sc + q] = i
                min_gap = min(min_gap, gap)
                if q == 0:
                    row += [al, (bl + br) / 2]
                else:
                    row += [al, (br - bl) * (math.gamma(2 / al) / math.gamma(1 / al)), bl, br]
        if ok:
            feat[b] = row
    return feat, index, min_gap


def score(feat, mu_p, cov_p):
    f = feat[np.isfinite(feat).all(axis=1)]
    if len(f) < 2:
        raise ValueError(f"niqe: {len(f)} block(s) with finite features; 2 are needed")
    mean = np.array([math.fsum(f[:, j].tolist()) / len(f) for j in range(f.shape[1])])
    c = f - mean
    cov = (c.T @ c) / (len(f) - 1)
    d = np.asarray(mu_p) - mean
    return float(math.sqrt(d @ np.linalg.pinv((np.asarray(cov_p) + cov) / 2.0) @ d))


def fit_model(images, B=96, mode="gray"):
    """-> (mu, cov, rows): blocks whose scale-1 sharpness exceeds 0.75 of their image's maximum."""
    rows = []
    for img in images:
        st, _, _ = stats(img, 0, B, mode)
        feat, _, _ = features(st, B)
        sharp = st[0, :, 25] / float(B * B)
        rows.append(feat[sharp > 0.75 * sharp.max()])
    f = np.concatenate(rows)
    f = f[np.isfinite(f).all(axis=1)]
    if len(f) < 2:
        raise ValueError("niqe fit: fewer than 2 rows")
    return f.mean(axis=0), np.cov(f, rowvar=False), len(f)


def niqe(img, mu_p, cov_p, shave=0, B=96, mode="gray"):
    st, _, _ = stats(img, shave, B, mode)
    return score(features(st, B)[0], mu_p, cov_p)
