"""Float64 restatements of the LPIPS head's gradient (docs/modes.md section 4o) for the tests, in numpy.

With na = sqrt(sum a^2), da = na + 1e-10, ah = a / da (likewise b), t = ah - bh, q = sum_c w_c t_c ah_c, per pixel of pair n:

    ga_j = (2 g[n] / (H W)) * (w_j t_j - (a_j / na) q) / da,        ga_j = 0 for every j where na == 0.

The second line is a DEFINITION: the formula's own value at such a pixel is 2 w_j t_j / 1e-10 and autograd's is NaN (the derivative of
the square root at zero); every channel of the pixel left its ReLU at zero, so the conv behind the tap masks the gradient anyway.

  grad_exact(fa, fb, w, g)     the formula, float64, every sum a math.fsum -> float64 [N,H,W,C]
  grad_bound(fa, fb, w, g)     how far the float64 value that grad_ordered rounds may be from grad_exact (its docstring)
  grad_ordered(fa, fb, w, g)   the IEEE operations of lpips_layer_bwd_kernel (pesr_amd/csrc/lpips.hip) in the kernel's order, ending in
                               ONE rounding to float32: what the device must equal bit for bit
  fp32_allowance(exact, bound) grad_bound plus that one rounding

fa, fb: [N, H, W, C] arrays of float32 values; w: [C]; g: [N] float64."""
import math

import numpy as np

import lpips_oracle as LO

EPS, U = LO.EPS, LO.U


def _exact_parts(fa, fb, w):
    a, b, w = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64), np.asarray(w, dtype=np.float64)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    na = np.array([math.sqrt(math.fsum(r * r)) for r in a2])          # (a float32 squared is exact in float64)
    nb = np.array([math.sqrt(math.fsum(r * r)) for r in b2])
    da, db = na + EPS, nb + EPS
    ah, bh = a2 / da[:, None], b2 / db[:, None]
    t = ah - bh
    wt = w[None, :] * t
    p = wt * ah
    q = np.array([math.fsum(r) for r in p])
    return a2, na, da, ah, bh, t, wt, p, q


def grad_exact(fa, fb, w, g):
    """-> float64 [N,H,W,C]."""
    shape = np.asarray(fa).shape
    a2, na, da, ah, bh, t, wt, p, q = _exact_parts(fa, fb, w)
    scale = np.repeat((2.0 * np.asarray(g, dtype=np.float64)) / float(shape[1] * shape[2]), shape[1] * shape[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = scale[:, None] * (wt - (a2 / na[:, None]) * q[:, None]) / da[:, None]
    out[na == 0] = 0.0
    return out.reshape(shape)


def grad_bound(fa, fb, w, g):
    """-> [N,H,W,C]: |x - grad_exact| is at most this, x the float64 value that grad_ordered rounds to float32.  u = 2^-53, K = C / 64;
    every operation is correctly rounded (relative error <= u), w and a are float32 values and exact in float64, and 2 g / (H W) is the
    same two operations on both sides.  The first five lines are lpips_oracle.head_bound's.
      sum of squares   the kernel's chain: K - 1 lane and 6 tree additions of non-negative terms, fsum one rounding: (K + 6) u apart.
      na               the square root halves that, each side rounds once: en = (K + 6) / 2 + 2.
      da = na + 1e-10  a positive constant only shrinks the relative difference, each side rounds once: e1 = en + 2.
      ah = a / da      each side rounds once: d_ah = (e1 + 2) u |ah|; the same for bh.
      t = ah - bh      THE CANCELLATION, absolute only: d_t = (e1 + 2) u (|ah| + |bh|) + 2 u |t|.
      wt = w t         d_wt = w d_t + 2 u |wt|.
      p = wt ah        d_p = |ah| d_wt + |wt| d_ah + 2 u |p|.
      q = sum p        signed terms: K + 5 additions in the kernel's chain, (K + 5) u sum |p|; fsum: u |q|:
                       d_q = sum d_p + (K + 5) u sum |p| + u |q|.
      m = a (q / na)   the kernel: r = q / na, m = a r; the formula: (a / na) q; two roundings each, na differs by en u:
                       d_m = (|a| / na) d_q + (en + 4) u |m|.
      v = wt - m       THE SECOND CANCELLATION (where a ~ b both terms are tiny and of one size): d_v = d_wt + d_m + 2 u |v|.
      times 2g/(HW)/da the kernel: c = scale / da, c v; the formula: (scale v) / da; two roundings each, da differs by e1 u:
    bound = (|scale| / da) d_v + (e1 + 4) u |grad_exact|, times 1 + 1e-6 for the products of two errors of size u.  0 where na == 0
    (both sides return the defined 0 there)."""
    shape = np.asarray(fa).shape
    hw = shape[1] * shape[2]
    a2, na, da, ah, bh, t, wt, p, q = _exact_parts(fa, fb, w)
    w = np.asarray(w, dtype=np.float64)[None, :]
    K = shape[3] // 64
    en = (K + 6) / 2 + 2
    e1 = en + 2
    d_ah = (e1 + 2) * U * np.abs(ah)
    d_t = (e1 + 2) * U * (np.abs(ah) + np.abs(bh)) + 2 * U * np.abs(t)
    d_wt = w * d_t + 2 * U * np.abs(wt)
    d_p = np.abs(ah) * d_wt + np.abs(wt) * d_ah + 2 * U * np.abs(p)
    d_q = d_p.sum(axis=1) + (K + 5) * U * np.abs(p).sum(axis=1) + U * np.abs(q)
    scale = np.repeat(np.abs(2.0 * np.asarray(g, dtype=np.float64)) / float(hw), hw)
    with np.errstate(divide="ignore", invalid="ignore"):
        a_na = np.abs(a2) / na[:, None]
        m = a_na * np.abs(q)[:, None]
        d_m = a_na * d_q[:, None] + (en + 4) * U * m
        v = wt - (a2 / na[:, None]) * q[:, None]
        d_v = d_wt + d_m + 2 * U * np.abs(v)
        exact = scale[:, None] * v / da[:, None]
        out = (scale / da)[:, None] * d_v + (e1 + 4) * U * np.abs(exact)
    out[na == 0] = 0.0
    return (out * (1 + 1e-6)).reshape(shape)


def fp32_allowance(exact, bound):
    """grad_bound plus ONE rounding to float32 of a value within `bound` of `exact`: half an ulp, 2^-24 relative in the normal range and
    2^-150 absolute below it."""
    return bound + 2.0 ** -24 * (np.abs(exact) + bound) + 2.0 ** -150


def grad_ordered(fa, fb, w, g):
    """-> float32 [N,H,W,C], the bits of pesr_lpips_layer_bwd."""
    a, b, w = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64), np.asarray(w, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    N, H, W, C = a.shape
    assert C in (64, 128, 256, 512) and b.shape == a.shape and w.shape == (C,) and g.shape == (N,)
    idx = LO.lane_channels(C)
    K = idx.shape[1]
    A, B, Wd = a[..., idx], b[..., idx], w[idx]                       # [N,H,W,64,K], [64,K]
    scale = ((2.0 * g) / float(H * W))[:, None, None]                # [N,1,1]
    sa, sb = np.zeros(A.shape[:-1]), np.zeros(A.shape[:-1])
    for k in range(K):
        sa = sa + A[..., k] * A[..., k]
        sb = sb + B[..., k] * B[..., k]
    na = np.sqrt(LO.wave_sum(sa, LO.ASCENDING))                       # [N,H,W]
    nb = np.sqrt(LO.wave_sum(sb, LO.ASCENDING))
    da, db = na + EPS, nb + EPS
    wt = np.zeros(A.shape)
    acc = np.zeros(A.shape[:-1])
    for k in range(K):
        ah = A[..., k] / da[..., None]
        bh = B[..., k] / db[..., None]
        t = ah - bh
        wt[..., k] = Wd[:, k] * t
        acc = acc + wt[..., k] * ah
    q = LO.wave_sum(acc, LO.ASCENDING)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = q / na
        c = scale / da
        out = np.zeros(a.shape, dtype=np.float32)
        for k in range(K):
            m = A[..., k] * r[..., None]
            v = wt[..., k] - m
            cv = c[..., None] * v
            out[..., idx[:, k]] = np.where((na == 0.0)[..., None], np.float32(0.0), cv.astype(np.float32))
    return out
