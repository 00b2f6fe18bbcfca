"""Float64 restatements of DISTS (docs/modes.md section 4t) for the tests: numpy for the head, torch on the CPU for the trunk.

  l2pool_f64(x)                       the L2 pooling in float64, a depthwise conv of x * x; L2POOL_RTOL bounds the fp32 kernel against it
  stats_exact(fa, fb)                 the five statistics in exact rational arithmetic, rounded once
  stats_bound(fa, fb)                 how far layer_ordered's statistics may be from stats_exact, from the counts of rounded operations
  layer_ordered(fa, fb, alpha, beta)  the IEEE operations of pesr_amd/csrc/dists.hip in the kernels' order: what the device must equal
                                      bit for bit
  dists_f64(a, b, tensors)            the whole metric, the definition: the trunk as torch float64 conv2d, the centred statistics
  dists_published(a, b, tensors)      a literal transcription of the published DISTS_pytorch forward, in float64
  dists_trunk32(...)                  dists_f64 with a float32 trunk (direct convs in one stated order, fp32 pooling), the statistics
                                      still float64

fa, fb: [N, H, W, C] arrays of float32 values; alpha, beta: [C] float64; tensors: DistsModel.tensors()."""
import math
from fractions import Fraction

import numpy as np

import lpips_oracle as LO

U = 2.0 ** -53
C1 = C2 = 1e-6
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CFG, TAPS = LO.CFG, LO.TAPS
STAGE_CHANNELS = (3, 64, 128, 256, 512, 512)
BLOCK_PIX, THREADS = 256, 256                                       # pixels per workgroup of the two passes; lanes of every kernel

# The fp32 kernel against l2pool_f64, relative to y, first order.  Under the root stand nine squares (one rounding each), eight additions
# and the + 1e-12; the weights are powers of two and round nothing.  All terms are non-negative, so nothing cancels: a term passes
# through its square, at most eight additions and the + 1e-12, which is at most 10 * 2^-24 relative to the sum under the root.  The root
# halves that and rounds once itself: 6 * 2^-24.  The kernel's count is the one this bound was stated for; 8 * 2^-24 is allowed.
L2POOL_RTOL = 8 * 2.0 ** -24


# ---- the L2 pooling ----------------------------------------------------------------------------------------------------------------
def _l2pool(h, dtype):
    """torch [M,C,H,W] in `dtype` -> sqrt(conv(h * h, g, stride 2, padding 1, depthwise) + 1e-12), [M,C,ceil(H/2),ceil(W/2)]."""
    import torch
    import torch.nn.functional as F
    a = torch.tensor([1.0, 2.0, 1.0], dtype=dtype)
    g = (a[:, None] * a[None, :] / 16).view(1, 1, 3, 3).repeat(h.shape[1], 1, 1, 1)
    return (F.conv2d(h * h, g, stride=2, padding=1, groups=h.shape[1]) + 1e-12).sqrt()


def l2pool_f64(x):
    """[N,H,W,C] float32 values -> float64 [N,ceil(H/2),ceil(W/2),C]."""
    import torch
    h = torch.as_tensor(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    return _l2pool(h, torch.float64).permute(0, 2, 3, 1).contiguous().numpy()


# ---- the statistics, exactly -------------------------------------------------------------------------------------------------------
def stats_exact(fa, fb):
    """-> [N, C, 5] (mu_a, mu_b, var_a, var_b, cov), each the exact rational value rounded once to float64.  Every float is a rational
    number, so sums and products of fractions.Fraction are exact; math.fsum of the float64 products a * a (exact for fp32 inputs) would
    give the raw moments correctly rounded, but var = E[a^2] - mu^2 then cancels at large means, which is what these tests are about."""
    a, b = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    N, H, W, C = a.shape
    P = H * W
    out = np.zeros((N, C, 5))
    for n in range(N):
        for c in range(C):
            xa = [Fraction(float(v)) for v in a[n, :, :, c].reshape(-1)]
            xb = [Fraction(float(v)) for v in b[n, :, :, c].reshape(-1)]
            ma, mb = sum(xa) / P, sum(xb) / P
            va = sum(v * v for v in xa) / P - ma * ma
            vb = sum(v * v for v in xb) / P - mb * mb
            cv = sum(p * q for p, q in zip(xa, xb)) / P - ma * mb
            out[n, c] = [float(ma), float(mb), float(va), float(vb), float(cv)]
    return out


def _depth(P):
    """The additions a value passes through on its way into a statistic, and the final division: at most 64 in a lane's chain of a
    block, 3 across the four waves, ceil(blocks / 256) in mean_partials_kernel's lane, 6 + 3 in its tree, 1 division."""
    nb = -(-P // BLOCK_PIX)
    return 64 + 3 + -(-nb // THREADS) + 9 + 1


def stats_bound(fa, fb):
    """-> [N, C, 5]: |layer_ordered's statistics - stats_exact| is at most this.  u = 2^-53, D = _depth(P), of order P for a small P.
      mu     a sum of P terms of either sign: every addition is within u of its result, whose size is at most the sum of |a|:
             D u mean(|a|), and u |mu| for the rounding of stats_exact itself.
      var    sum((a - m)^2) / P = var + (m - mu)^2 for ANY m, so the kernel's rounded mean m costs d_mu^2, second order.  a - m rounds
             once, its square once more: 3 u on each term; the terms are non-negative, so the sum adds D u: (D + 4) u (var + d_mu^2),
             with the rounding of stats_exact.
      cov    the same with |da db| in the place of da^2, and mean(|da db|) <= sqrt(var_a var_b):
             (D + 4) u sqrt((var_a + d_a^2)(var_b + d_b^2)) + d_a d_b + u |cov|.
    Each carries a factor 1 + 1e-6 for the products of two errors of size u."""
    a, b = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    N, H, W, C = a.shape
    D = _depth(H * W)
    ex = stats_exact(fa, fb)
    absa, absb = np.abs(a).mean(axis=(1, 2)), np.abs(b).mean(axis=(1, 2))
    out = np.zeros((N, C, 5))
    out[..., 0] = D * U * absa + U * np.abs(ex[..., 0])
    out[..., 1] = D * U * absb + U * np.abs(ex[..., 1])
    va, vb = ex[..., 2] + out[..., 0] ** 2, ex[..., 3] + out[..., 1] ** 2
    out[..., 2] = (D + 4) * U * va + out[..., 0] ** 2
    out[..., 3] = (D + 4) * U * vb + out[..., 1] ** 2
    out[..., 4] = (D + 4) * U * np.sqrt(va * vb) + out[..., 0] * out[..., 1] + U * np.abs(ex[..., 4])
    return out * (1 + 1e-6)


def stats_uncentred(fa, fb):
    """The one-pass form the kernel must NOT use, var = mean(a^2) - mu^2 and cov = mean(a b) - mu_a mu_b in float64: here to show on
    the CPU that it misses stats_bound at a large mean.  -> [N, C, 5]."""
    a, b = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    ma, mb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    return np.stack([ma, mb, (a * a).mean(axis=(1, 2)) - ma * ma, (b * b).mean(axis=(1, 2)) - mb * mb,
                     (a * b).mean(axis=(1, 2)) - ma * mb], axis=-1)


# ---- the kernels' order ------------------------------------------------------------------------------------------------------------
def _block_partials(x):
    """x: [N, P, C] float64 terms -> [N, C, blocks]: wave v of a block adds the block's pixels v, v + 4, v + 8, ... in ascending order
    from 0.0 (pixels past the image are skipped), then ((s0 + s1) + s2) + s3."""
    N, P, C = x.shape
    nb = -(-P // BLOCK_PIX)
    pad = np.zeros((N, nb * BLOCK_PIX, C))
    pad[:, :P] = x
    px = pad.reshape(N, nb, BLOCK_PIX // 4, 4, C)                     # pixel 4 i + v of the block at [i][v]
    valid = (np.arange(nb * BLOCK_PIX) < P).reshape(nb, BLOCK_PIX // 4, 4)
    s = np.zeros((N, nb, 4, C))
    for i in range(BLOCK_PIX // 4):
        s = np.where(valid[None, :, i, :, None], s + px[:, :, i], s)
    part = ((s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]) + s[:, :, 3]     # [N, nb, C]
    return part.transpose(0, 2, 1)


def _block_sum(ls):
    """block_sum_d of common.h over the last axis of 256 lanes: wave_sum_d (offsets 32 .. 1) in each wave, then ((r0 + r1) + r2) + r3."""
    r4 = LO.wave_sum(ls.reshape(ls.shape[:-1] + (THREADS // 64, 64)), LO.DESCENDING)
    return ((r4[..., 0] + r4[..., 1]) + r4[..., 2]) + r4[..., 3]


def _mean_partials(part, count):
    """mean_partials_kernel of reduce.hip over the last axis: lane t adds partials t, t + 256, ... ascending from 0.0, block_sum_d,
    one division."""
    nb = part.shape[-1]
    rounds = -(-nb // THREADS)
    pp = np.zeros(part.shape[:-1] + (rounds * THREADS,))
    pp[..., :nb] = part
    pv = (np.arange(rounds * THREADS) < nb).reshape(rounds, THREADS)
    pp = pp.reshape(part.shape[:-1] + (rounds, THREADS))
    ls = np.zeros(part.shape[:-1] + (THREADS,))
    for r in range(rounds):
        ls = np.where(pv[r], ls + pp[..., r, :], ls)
    return _block_sum(ls) / float(count)


def layer_ordered(fa, fb, alpha, beta):
    """-> (contribution [N], statistics [N, C, 5]), the bits of pesr_dists_layer."""
    a, b = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    N, H, W, C = a.shape
    assert C in (3, 64, 128, 256, 512) and b.shape == a.shape and alpha.shape == beta.shape == (C,)
    P = H * W
    a, b = a.reshape(N, P, C), b.reshape(N, P, C)
    ma, mb = _mean_partials(_block_partials(a), P), _mean_partials(_block_partials(b), P)     # [N, C]
    da, db = a - ma[:, None, :], b - mb[:, None, :]
    va = _mean_partials(_block_partials(da * da), P)
    vb = _mean_partials(_block_partials(db * db), P)
    cv = _mean_partials(_block_partials(da * db), P)
    m = ma * mb
    s1 = (2.0 * m + C1) / ((ma * ma + mb * mb) + C1)
    s2 = (2.0 * cv + C2) / ((va + vb) + C2)
    term = alpha * s1 + beta * s2                                     # [N, C]
    rounds = -(-C // THREADS)
    tp = np.zeros((N, rounds * THREADS))
    tp[:, :C] = term
    tv = (np.arange(rounds * THREADS) < C).reshape(rounds, THREADS)
    tp = tp.reshape(N, rounds, THREADS)
    acc = np.zeros((N, THREADS))
    for r in range(rounds):                                           # lane t: channels t, t + 256, ...
        acc = np.where(tv[r], acc + tp[:, r], acc)
    return _block_sum(acc), np.stack([ma, mb, va, vb, cv], axis=-1)


# ---- the whole metric --------------------------------------------------------------------------------------------------------------
def weight_sum(tensors):
    """w = sum(alpha) + sum(beta): the exactly rounded sum of the 2950 values (math.fsum: no order to state)."""
    return math.fsum(tensors["alpha"].tolist() + tensors["beta"].tolist())


def stages(x, tensors, dtype):
    """[M,3,H,W] torch tensor of 0..255 values -> the six stage tensors [M,C,h,w] in `dtype` (direct convs on the CPU)."""
    import torch
    import torch.nn.functional as F
    x = x.to(dtype) / 255
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    h = (x - mean) / std
    out, i = [x], 0
    for v in CFG:
        if v == "M":
            h = _l2pool(h, dtype)
            continue
        h = F.relu(F.conv2d(h, tensors[f"conv{i}.weight"].to(dtype), tensors[f"conv{i}.bias"].to(dtype), padding=1))
        if i in TAPS:
            out.append(h)
        i += 1
    return out


def _conv3x3_f32(x, w, b):
    """A direct 3 x 3 conv, padding 1, in float32 with one rounding per operation and ONE order on every machine: the bias, then
    acc = acc + w * x over the input channels and, inside a channel, the nine taps, ascending (no BLAS, whose order is its own)."""
    M, Cin, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.broadcast_to(b[None, :, None, None], (M, w.shape[0], H, W)).astype(np.float32)
    for ci in range(Cin):
        for ky in range(3):
            for kx in range(3):
                acc += w[None, :, ci, ky, kx, None, None] * xp[:, ci:ci + 1, ky:ky + H, kx:kx + W]
    return acc


def _l2pool_f32(x):
    """The L2 pooling in float32, one rounding per operation, the window's taps in ascending order."""
    M, C, H, W = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    xp = np.pad(x * x, ((0, 0), (0, 0), (1, 2), (1, 2)))
    acc = np.zeros((M, C, Ho, Wo), np.float32)
    for ky in range(3):
        for kx in range(3):
            g = np.float32((1, 2, 1)[ky] * (1, 2, 1)[kx] / 16.0)
            acc += g * xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    return np.sqrt(acc + np.float32(1e-12))


def stages32(x, tensors):
    """stages() in float32 by the two functions above: the same values on every machine, which the recorded measurement of
    tests/dists_cases.py needs.  -> six float32 torch tensors."""
    import torch
    x = np.asarray(x, dtype=np.float32) / np.float32(255)
    h = (x - np.array(MEAN, np.float32).reshape(1, 3, 1, 1)) / np.array(STD, np.float32).reshape(1, 3, 1, 1)
    out, i = [x], 0
    for v in CFG:
        if v == "M":
            h = _l2pool_f32(h)
            continue
        h = np.maximum(_conv3x3_f32(h, tensors[f"conv{i}.weight"].numpy(), tensors[f"conv{i}.bias"].numpy()), np.float32(0))
        if i in TAPS:
            out.append(h)
        i += 1
    assert all(t.dtype == np.float32 for t in out)
    return [torch.from_numpy(t) for t in out]


def _crop(a, b, shave):
    import torch
    a, b = torch.as_tensor(np.array(a)), torch.as_tensor(np.array(b))
    H, W = a.shape[2], a.shape[3]
    return a[:, :, shave:H - shave, shave:W - shave], b[:, :, shave:H - shave, shave:W - shave]


def _metric(a, b, tensors, shave, dtype):
    """-> (score [N], the six stage contributions [6, N]), float64."""
    import torch
    a, b = _crop(a, b, shave)
    n = a.shape[0]
    w = weight_sum(tensors)
    aw, bw = tensors["alpha"].to(torch.float64) / w, tensors["beta"].to(torch.float64) / w
    parts, c0 = [], 0
    with torch.no_grad():
        x = torch.cat([a, b])
        for f in (stages32(x.numpy(), tensors) if dtype == torch.float32 else stages(x, tensors, dtype)):
            f = f.to(torch.float64)
            fa, fb = f[:n], f[n:]
            c = f.shape[1]
            ma, mb = fa.mean(dim=(2, 3), keepdim=True), fb.mean(dim=(2, 3), keepdim=True)
            va, vb = ((fa - ma) ** 2).mean(dim=(2, 3)), ((fb - mb) ** 2).mean(dim=(2, 3))
            cv = ((fa - ma) * (fb - mb)).mean(dim=(2, 3))
            ma, mb = ma[:, :, 0, 0], mb[:, :, 0, 0]
            s1 = (2 * ma * mb + C1) / (ma * ma + mb * mb + C1)
            s2 = (2 * cv + C2) / (va + vb + C2)
            parts.append((aw[c0:c0 + c] * s1 + bw[c0:c0 + c] * s2).sum(dim=1))
            c0 += c
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return (1.0 - total).numpy(), torch.stack(parts).numpy()


def dists_f64(a, b, tensors, shave=0, return_parts=False):
    """-> float64 [N] (and the six stage contributions [6, N])."""
    import torch
    score, parts = _metric(a, b, tensors, shave, torch.float64)
    return (score, parts) if return_parts else score


def dists_trunk32(a, b, tensors, shave=0):
    """-> float64 [N], the trunk (the image / 255, the convs, the pooling) in float32."""
    import torch
    return _metric(a, b, tensors, shave, torch.float32)[0]


def dists_published(a, b, tensors, shave=0):
    """The forward of the published DISTS_pytorch package, transcribed literally (x_var = mean((x - mean)^2), xy_cov = mean(x y) -
    mean_x mean_y, the weights split per stage after the division by their sum, dist1 and dist2 accumulated apart), in float64."""
    import torch
    a, b = _crop(a, b, shave)
    with torch.no_grad():
        feats0 = stages(a, tensors, torch.float64)
        feats1 = stages(b, tensors, torch.float64)
        alpha_, beta_ = tensors["alpha"].to(torch.float64).view(1, -1, 1, 1), tensors["beta"].to(torch.float64).view(1, -1, 1, 1)
        dist1, dist2 = 0, 0
        c1, c2 = 1e-6, 1e-6
        w_sum = alpha_.sum() + beta_.sum()
        alpha = torch.split(alpha_ / w_sum, STAGE_CHANNELS, dim=1)
        beta = torch.split(beta_ / w_sum, STAGE_CHANNELS, dim=1)
        for k in range(len(STAGE_CHANNELS)):
            x_mean = feats0[k].mean([2, 3], keepdim=True)
            y_mean = feats1[k].mean([2, 3], keepdim=True)
            S1 = (2 * x_mean * y_mean + c1) / (x_mean ** 2 + y_mean ** 2 + c1)
            dist1 = dist1 + (alpha[k] * S1).sum(1, keepdim=True)
            x_var = ((feats0[k] - x_mean) ** 2).mean([2, 3], keepdim=True)
            y_var = ((feats1[k] - y_mean) ** 2).mean([2, 3], keepdim=True)
            xy_cov = (feats0[k] * feats1[k]).mean([2, 3], keepdim=True) - x_mean * y_mean
            S2 = (2 * xy_cov + c2) / (x_var + y_var + c2)
            dist2 = dist2 + (beta[k] * S2).sum(1, keepdim=True)
        score = 1 - (dist1 + dist2).reshape(-1)
    return score.numpy()
