"""CPU restatement of the HBM-bound kernels of every train step - adam.hip, elementwise.hip, loss.hip - written from what each
operation means and sharing no code with pesr_amd.  TEST INFRASTRUCTURE; no GPU import.

Every function computes in the dtype of the tensors it is given: float64 tensors give the reference, float32 tensors give "the
fp32 evaluation of the same expression" that the exact-equality tests compare with.  Activation tensors are NHWC, [N, H, W, C], as
the kernels take them.  Selections (max-pool, masks) are exact in any dtype.
"""
import math

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------
# Adam (torch.optim.Adam, single-tensor order, no weight decay, no amsgrad; the header of adam.hip)
# ------------------------------------------------------------------------------------------------
def adam_scalars(lr, b1, b2, step):
    """-> (lr / bc1, sqrt(bc2)) in float64 for the 1-based step count."""
    bc1 = 1.0 - float(b1) ** float(step)
    bc2 = 1.0 - float(b2) ** float(step)
    return float(lr) / bc1, math.sqrt(bc2)


def adam_moments(m, v, g, b1, b2, gscale=1.0):
    """-> (m', v'): m' = lerp(m, G, 1 - b1), v' = b2 v + (1 - b2) G G with G = gscale * g (the gradient is scaled first)."""
    G = g.to(m.dtype) * gscale
    return m + (G - m) * (1.0 - b1), v * b2 + G * G * (1.0 - b2)


def adam_param(p, m_new, v_new, step_size, bc2_sqrt, eps):
    """-> (p', update, den): p' = p - step_size * m' / (sqrt(v') / sqrt(bc2) + eps)."""
    den = v_new.sqrt() / bc2_sqrt + eps
    upd = step_size * (m_new / den)
    return p - upd, upd, den


def adam_step(p, m, v, g, b1, b2, eps, step_size, bc2_sqrt, gscale=1.0):
    """One step -> (p', m', v')."""
    m2, v2 = adam_moments(m, v, g, b1, b2, gscale)
    return adam_param(p, m2, v2, step_size, bc2_sqrt, eps)[0], m2, v2


# ------------------------------------------------------------------------------------------------
# L1 + total variation on sr, hr [N, H, W, 3]; MSE
# ------------------------------------------------------------------------------------------------
def l1_tv_terms(sr, hr):
    """-> (|sr - hr|, |horizontal differences|, |vertical differences|): the terms of the two sums."""
    return (sr - hr).abs(), (sr[:, :, :-1] - sr[:, :, 1:]).abs(), (sr[:, :-1] - sr[:, 1:]).abs()


def l1_tv_value(sr, hr):
    """-> [mean |sr - hr|, SUM |sr[.., x] - sr[.., x+1]| + SUM |sr[y] - sr[y+1]|]  (F.l1_loss and oracle/step.py::tv_loss)."""
    a, h, v = l1_tv_terms(sr, hr)
    return torch.stack([a.mean(), h.sum() + v.sum()])


def tv_sign_count(sr):
    """d(tv)/d(sr): every pixel is the minuend of the difference with its right and lower neighbour and the subtrahend of the
    difference with its left and upper one; each contributes the sign of that difference, sign(0) = 0.  Integer-valued, in -4 .. 4."""
    t = torch.zeros_like(sr)
    sh = torch.sign(sr[:, :, :-1] - sr[:, :, 1:])
    sv = torch.sign(sr[:, :-1] - sr[:, 1:])
    t[:, :, :-1] += sh
    t[:, :, 1:] -= sh
    t[:, :-1] += sv
    t[:, 1:] -= sv
    return t


def l1_tv_grad(sr, hr, g_l1, g_tv):
    """g_l1 * sign(sr - hr) + g_tv * d(tv)/d(sr), sign(0) = 0; g_l1 carries the 1 / numel of the mean."""
    return g_l1 * torch.sign(sr - hr) + g_tv * tv_sign_count(sr)


def mse_value(a, b):
    return ((a - b) ** 2).mean()


def mse_grad(a, b, gscale):
    return (a - b) * gscale


# ------------------------------------------------------------------------------------------------
# MeanShift, a 1x1 conv on 3 channels: y[.., i] = sum_j w[i][j] x[.., j] + b[i], x [N, H, W, 3]
# ------------------------------------------------------------------------------------------------
def meanshift_fwd(x, w, b):
    return x @ w.reshape(3, 3).t() + b


def meanshift_bwd(dy, x, w):
    """-> (dx [N,H,W,3], dw [3,3], db [3]) for dy [N,H,W,3]."""
    g, xs = dy.reshape(-1, 3), x.reshape(-1, 3)
    return dy @ w.reshape(3, 3), g.t() @ xs, g.sum(0)


# ------------------------------------------------------------------------------------------------
# 2x2 / 2 max-pool, floor mode, x [N, H, W, C]
# ------------------------------------------------------------------------------------------------
def _windows(x):
    """The four window positions in row-major order, each [N, H//2, W//2, C]; the last row / column of an odd side is left out."""
    H2, W2 = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    x = x[:, :H2, :W2]
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def maxpool_fwd(x):
    a, b, c, d = _windows(x)
    return torch.maximum(torch.maximum(a, b), torch.maximum(c, d))


def maxpool_winners(x):
    """-> four boolean masks: where each window position is the FIRST one, in row-major order, to equal the window's maximum."""
    a, b, c, d = _windows(x)
    m = maxpool_fwd(x)
    wa = a == m
    wb = (b == m) & ~wa
    wc = (c == m) & ~wa & ~wb
    wd = ~wa & ~wb & ~wc
    return wa, wb, wc, wd


def maxpool_bwd(x, dy, relu_in):
    """dx [N,H,W,C] (even sides): dy goes to the first maximum of its window; with relu_in only where that maximum is > 0 (the pool
    follows a ReLU whose input x is: max_pool(relu(x)) lets a gradient through only at a positive maximum)."""
    dx = torch.zeros_like(x)
    g = dy * (maxpool_fwd(x) > 0) if relu_in else dy
    for (oy, ox), wmask in zip(((0, 0), (0, 1), (1, 0), (1, 1)), maxpool_winners(x)):
        dx[:, oy::2, ox::2] = g * wmask
    return dx


def maxpool_tied_windows(x):
    """Number of windows whose maximum is attained more than once, and the number of windows."""
    a, b, c, d = _windows(x)
    m = maxpool_fwd(x)
    hits = (a == m).int() + (b == m).int() + (c == m).int() + (d == m).int()
    return int((hits > 1).sum()), m.numel()


# ------------------------------------------------------------------------------------------------
# (Leaky)ReLU masking with an optional scale and an optional addend
# ------------------------------------------------------------------------------------------------
def relu_mask(g, ref=None, add=None, alpha=1.0, slope=0.0):
    """out = (ref > 0 ? alpha g : slope alpha g) + add; without ref nothing is masked, without add nothing is added.  "Not > 0" takes
    the slope: 0.0 and -0.0 do."""
    alpha, slope = torch.tensor(alpha, dtype=g.dtype), torch.tensor(slope, dtype=g.dtype)     # the scalars in the tensors' precision
    v = g * alpha
    if ref is not None:
        v = torch.where(ref > 0, v, v * slope)
    return v if add is None else v + add


# ------------------------------------------------------------------------------------------------
# GAN losses on the logits r (real), f (fake), [B, 1]  (oracle/step.py::focal_loss and BCE-with-logits)
# ------------------------------------------------------------------------------------------------
def focal_loss(x, t, gamma):
    """oracle/step.py::focal_loss, restated so it runs in the dtype of x."""
    p = torch.sigmoid(x)
    pt = p * t + (1 - p) * (1 - t)
    w = (1 - pt).pow(gamma)
    return (w * F.binary_cross_entropy_with_logits(x, t, reduction="none")).mean()


def gan_loss(r, f, gan_type, side, focal, gamma):
    """side 0: the discriminator's loss (always plain BCE); side 1: the generator's (focal: FocalLoss with that gamma)."""
    ones, zeros = torch.ones_like(r), torch.zeros_like(r)
    bce = F.binary_cross_entropy_with_logits
    lf = (lambda z, t: focal_loss(z, t, gamma)) if focal else bce
    if side == 0:
        return {"SGAN": lambda: bce(r, ones) + bce(f, zeros), "RSGAN": lambda: bce(r - f, ones),
                "RaSGAN": lambda: 0.5 * (bce(r - f.mean(), ones) + bce(f - r.mean(), zeros))}[gan_type]()
    return {"SGAN": lambda: lf(f, ones), "RSGAN": lambda: lf(f - r, ones),
            "RaSGAN": lambda: 0.5 * (lf(r - f.mean(), zeros) + lf(f - r.mean(), ones))}[gan_type]()


def gan_loss_and_grads(r, f, gan_type, side, focal, gamma, scale):
    """-> (scale * loss, d/dr, d/df) by autograd in the dtype of r, f; a logit the loss does not depend on gets zeros."""
    r = r.detach().clone().requires_grad_(True)
    f = f.detach().clone().requires_grad_(True)
    val = gan_loss(r, f, gan_type, side, focal, gamma) * scale
    val.backward()
    return val.detach(), (r.grad if r.grad is not None else torch.zeros_like(r)), (f.grad if f.grad is not None else torch.zeros_like(f))


GAN_CASES = [(g, s, fo, ga) for g in ("SGAN", "RSGAN", "RaSGAN")
             for s, fo, ga in ((0, False, 1.0), (1, False, 1.0), (1, True, 1.0), (1, True, 2.0), (1, True, 0.0))]


def gan_logits(B, seed=7):
    """Logits of spread 4 with saturated entries at the start and at the end of the vectors (the first and the last wave of the block)."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.randn(B, 1, generator=gen) * 4
    f = torch.randn(B, 1, generator=gen) * 4
    for vec, at, val in ((r, 0, 30.0), (f, 1, -40.0), (r, 2, -25.0), (f, B - 1, 35.0), (r, B - 2, -30.0), (f, B - 3, -40.0)):
        if 0 <= at < B:
            vec[at] = val
    return r, f


# ------------------------------------------------------------------------------------------------
# tie-dense inputs
# ------------------------------------------------------------------------------------------------
def tied_pool_input(shape, seed):
    """[N, H, W, C] of integer-valued draws from {-1, 0, 1, 2} with one -0.0."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 3, shape, generator=gen).float()
    flat = x.view(-1)
    zeros = (flat == 0).nonzero()
    flat[int(zeros[len(zeros) // 2])] = -0.0
    return x


def tied_images(shape, seed):
    """sr, hr [N, H, W, 3], integer-valued in 0 .. 3: a quarter of the elements have sr == hr, a quarter of the neighbours are equal."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, shape, generator=gen).float(), torch.randint(0, 4, shape, generator=gen).float()
