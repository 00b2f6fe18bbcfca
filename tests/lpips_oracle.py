"""Float64 restatements of LPIPS (docs/modes.md section 4n) for the tests: numpy for the head, torch on the CPU for the trunk.

  head_exact(fa, fb, w)     the definition, every sum a math.fsum (exactly summed, rounded once)
  head_bound(fa, fb, w)     how far head_ordered may be from head_exact, from the counts of rounded operations (its docstring)
  head_ordered(fa, fb, w)   the IEEE operations of pesr_amd/csrc/lpips.hip in the kernel's order: what the device must equal bit for bit
  lpips_f64(a, b, tensors)  the whole metric, the trunk as torch float64 conv2d / max_pool2d
  lpips_trunk32(...)        the same with a float32 trunk (direct convs), the head still float64: the yardstick of fp32 conv rounding

fa, fb: [N, H, W, C] arrays of float32 values; w: [C]; tensors: LpipsModel.tensors()."""
import math

import numpy as np

EPS = 1e-10
U = 2.0 ** -53
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)
WG_PIX, WAVE_PIX, THREADS = 64, 16, 256


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _exact_parts(fa, fb, w):
    """-> (d [N,H,W], ahat, bhat, t [N,H,W,C]): norms from exactly summed squares, terms w * t * t exactly summed."""
    a, b, w = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64), np.asarray(w, dtype=np.float64)
    shape = a.shape[:-1]
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    na = np.array([math.sqrt(math.fsum(r * r)) for r in a2])          # (a float32 squared is exact in float64)
    nb = np.array([math.sqrt(math.fsum(r * r)) for r in b2])
    ah, bh = a2 / (na + EPS)[:, None], b2 / (nb + EPS)[:, None]
    t = ah - bh
    d = np.array([math.fsum(r) for r in w[None, :] * (t * t)])
    return d.reshape(shape), ah.reshape(a.shape), bh.reshape(a.shape), t.reshape(a.shape)


def head_exact(fa, fb, w):
    """-> (score [N], map [N,H,W])."""
    d = _exact_parts(fa, fb, w)[0]
    return np.array([math.fsum(m.reshape(-1)) / m.size for m in d]), d


def head_bound(fa, fb, w):
    """-> (score bound [N], map bound [N,H,W]): |head_ordered - head_exact| is at most this.  u = 2^-53, K = C / 64.  Every
    operation below is correctly rounded (relative error <= u); a float32 squared is exact in float64.
      sum of squares   all terms >= 0.  The kernel's chain has K - 1 lane additions and 6 tree additions, so it is within (K + 5) u
                       of the exact sum; fsum is within u: (K + 6) u between the two.
      norm             the square root halves that and each side rounds once: (K + 6) / 2 u + 2 u.
      + 1e-10          a positive constant only shrinks the relative difference, and each side rounds once: e1 = (K + 6) / 2 + 4.
      a / (na + eps)   each side rounds once: |ahat_ord - ahat_ex| <= (e1 + 2) u |ahat|, and the same for b.
      t = ahat - bhat  THE CANCELLATION: only the absolute error is bounded, dt = (e1 + 2) u (|ahat| + |bhat|) + 2 u |t|.
      w * (t * t)      |t_ord^2 - t_ex^2| <= 2 |t| dt + dt^2; the square and the product round once on each side: + 4 u w t^2.
      sum over c       terms >= 0: (K + 5) u for the kernel's chain and u for fsum, of d.
    map bound = sum_c w_c (2 |t_c| dt_c + dt_c^2) + (4 + K + 6) u d.
    score            the mean of non-negative d(p): the kernel adds at most 16 (wave) + 3 (workgroup) + ceil(groups / 256) (final lane)
                     + 6 + 3 (final tree) times and divides once; fsum and its division round twice:
    score bound = mean(map bound) + (31 + ceil(groups / 256)) u score.
    Both carry a factor 1 + 1e-6 for the second-order terms (products of two errors of size u)."""
    d, ah, bh, t = _exact_parts(fa, fb, w)
    w = np.asarray(w, dtype=np.float64)
    K = w.shape[0] // 64
    e1 = (K + 6) / 2 + 4
    dt = (e1 + 2) * U * (np.abs(ah) + np.abs(bh)) + 2 * U * np.abs(t)
    mb = (w * (2 * np.abs(t) * dt + dt * dt)).sum(axis=-1) + (4 + K + 6) * U * d
    mb = mb * (1 + 1e-6)
    hw = d.shape[1] * d.shape[2]
    groups = -(-hw // WG_PIX)
    score = np.array([math.fsum(m.reshape(-1)) / m.size for m in d])
    sb = mb.reshape(d.shape[0], -1).mean(axis=1) + (31 + -(-groups // THREADS)) * U * score
    return sb * (1 + 1e-6), mb


# ---- the kernel's order ------------------------------------------------------------------------------------------------------------
def lane_channels(C):
    """[64, K]: the channels lane l holds, in the order it adds them: C = 64: l; 128: 2l + e; 256: 4l + e; 512: 256 j + 4l + e."""
    K = C // 64
    V = min(K, 4)
    l, k = np.arange(64)[:, None], np.arange(K)[None, :]
    return (k // V) * 64 * V + l * V + (k % V)


ASCENDING, DESCENDING = (1, 2, 4, 8, 16, 32), (32, 16, 8, 4, 2, 1)


def wave_sum(v, offs):
    """A sum across the 64 lanes of the last axis: v = v + v[lane ^ off] for off in offs (ascending in the pixel kernel, descending
    in the final one).  Every lane ends with the same bits."""
    lane = np.arange(64)
    for off in offs:
        v = v + v[..., lane ^ off]
    assert bool((v == v[..., :1]).all())
    return v[..., 0]


def head_ordered(fa, fb, w):
    """-> (score [N], map [N,H,W]), the bits of pesr_lpips_layer."""
    a, b, w = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, H, W, C = a.shape
    assert C in (64, 128, 256, 512) and b.shape == a.shape and w.shape == (C,)
    idx = lane_channels(C)
    K = idx.shape[1]
    A, B, Wd = a[..., idx], b[..., idx], w[idx]                       # [N,H,W,64,K], [64,K]
    sa, sb = np.zeros(A.shape[:-1]), np.zeros(A.shape[:-1])
    for k in range(K):
        sa = sa + A[..., k] * A[..., k]
        sb = sb + B[..., k] * B[..., k]
    da = (np.sqrt(wave_sum(sa, ASCENDING)) + EPS)[..., None]
    db = (np.sqrt(wave_sum(sb, ASCENDING)) + EPS)[..., None]
    acc = np.zeros(A.shape[:-1])
    for k in range(K):
        t = A[..., k] / da - B[..., k] / db
        acc = acc + Wd[:, k] * (t * t)
    d = wave_sum(acc, ASCENDING)                                                 # [N,H,W]
    hw = H * W
    groups = -(-hw // WG_PIX)
    flat = np.zeros((N, groups * WG_PIX))
    flat[:, :hw] = d.reshape(N, hw)
    valid = (np.arange(groups * WG_PIX) < hw).reshape(groups, WG_PIX // WAVE_PIX, WAVE_PIX)
    px = flat.reshape(N, groups, WG_PIX // WAVE_PIX, WAVE_PIX)
    s = np.zeros(px.shape[:-1])
    for i in range(WAVE_PIX):                                         # a wave's pixels in ascending order; pixels past the image are skipped
        s = np.where(valid[None, ..., i], s + px[..., i], s)
    part = ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]          # [N, groups]
    rounds = -(-groups // THREADS)
    pp = np.zeros((N, rounds * THREADS))
    pp[:, :groups] = part
    pv = (np.arange(rounds * THREADS) < groups).reshape(rounds, THREADS)
    pp = pp.reshape(N, rounds, THREADS)
    ls = np.zeros((N, THREADS))
    for r in range(rounds):                                           # lane t: partials t, t + 256, ...
        ls = np.where(pv[None, r], ls + pp[:, r], ls)
    r4 = wave_sum(ls.reshape(N, THREADS // 64, 64), DESCENDING)
    score = (((r4[:, 0] + r4[:, 1]) + r4[:, 2]) + r4[:, 3]) / float(hw)
    return score, d


def head_five_sums(fa, fb, w):
    """The one-pass expansion the kernel must NOT use: d = S_waa / na'^2 + S_wbb / nb'^2 - 2 S_wab / (na' nb') from five sums per
    pixel, in float64.  Here to show on the CPU that it fails head_bound where a ~ b.  -> map [N,H,W]."""
    a, b, w = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64), np.asarray(w, dtype=np.float64)
    da, db = np.sqrt((a * a).sum(-1)) + EPS, np.sqrt((b * b).sum(-1)) + EPS
    return (w * a * a).sum(-1) / (da * da) + (w * b * b).sum(-1) / (db * db) - 2 * (w * a * b).sum(-1) / (da * db)


# ---- the whole metric --------------------------------------------------------------------------------------------------------------
def trunk(x, tensors, dtype):
    """[M,3,H,W] torch tensor of 0..255 values -> the five tapped feature maps [M,C,h,w] in `dtype` (direct convs on the CPU)."""
    import torch
    import torch.nn.functional as F
    x = x.to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    h = ((x / 127.5 - 1) - shift) / scale
    taps, i = [], 0
    for v in CFG:
        if v == "M":
            h = F.max_pool2d(h, 2)
            continue
        h = F.relu(F.conv2d(h, tensors[f"conv{i}.weight"].to(dtype), tensors[f"conv{i}.bias"].to(dtype), padding=1))
        if i in TAPS:
            taps.append(h)
        i += 1
    return taps


def _metric(a, b, tensors, shave, dtype):
    import torch
    a, b = torch.as_tensor(np.array(a)), torch.as_tensor(np.array(b))
    H, W = a.shape[2], a.shape[3]
    a, b = a[:, :, shave:H - shave, shave:W - shave], b[:, :, shave:H - shave, shave:W - shave]
    n = a.shape[0]
    with torch.no_grad():
        total = torch.zeros(n, dtype=torch.float64)
        for l, f in enumerate(trunk(torch.cat([a, b]), tensors, dtype)):
            f = f.to(torch.float64)
            fa, fb = f[:n], f[n:]
            ah = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + EPS)
            bh = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + EPS)
            w = tensors[f"lin{l}"].to(torch.float64).view(1, -1, 1, 1)
            total = total + (w * (ah - bh).pow(2)).sum(1).mean(dim=(1, 2))
    return total.numpy()


def lpips_f64(a, b, tensors, shave=0):
    """-> float64 [N]."""
    import torch
    return _metric(a, b, tensors, shave, torch.float64)


def lpips_trunk32(a, b, tensors, shave=0):
    """-> float64 [N], the trunk in float32."""
    import torch
    return _metric(a, b, tensors, shave, torch.float32)
