"""CPU restatement of pesr_amd/csrc/bn.hip - BatchNorm2d + LeakyReLU, training and eval mode, its backward and the backward of its
training backward - written from what each operation means and sharing no code with pesr_amd.  TEST INFRASTRUCTURE; no GPU import.

Every function computes in the dtype of the tensors it is given: float64 tensors give the reference.  Activations are NHWC,
[N, H, W, C]; per-channel quantities are [C] and reduce over the M = N * H * W rows.  The "fed" use: the apply and backward functions
take mean and invstd as arguments, so a test may hand them the kernel's own fp32 statistics (cast to float64) and bound the
elementwise pass without carrying the statistics' error.
"""
import torch

ROWS = (0, 1, 2)


def rows(x):
    return x.shape[0] * x.shape[1] * x.shape[2]


# ------------------------------------------------------------------------------------------------
# statistics
# ------------------------------------------------------------------------------------------------
def batch_stats(x, eps):
    """-> (mean, biased variance, invstd = 1 / sqrt(var + eps)) per channel.  Two-pass (mean first): no cancellation."""
    mean = x.mean(ROWS)
    var = ((x - mean) ** 2).mean(ROWS)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def running_update(running_mean, running_var, num_batches, mean, var, M, momentum):
    """nn.BatchNorm2d's update -> (running_mean', running_var', num_batches + 1): the UNBIASED variance var * M / (M - 1) goes into
    running_var.  At M = 1, where torch refuses to train, the factor is defined as 1 (bn.hip's `M > 1` guard)."""
    unb = var * (M / (M - 1.0)) if M > 1 else var
    return (1.0 - momentum) * running_mean + momentum * mean, (1.0 - momentum) * running_var + momentum * unb, num_batches + 1


def stats_from_part(part, M, eps):
    """part [rows][2][C] = per-row sums of x and of x * x -> (mean, var, invstd) as pesr_bn_finalize must make them: var = E[x^2] - mean^2,
    clamped at 0."""
    s = part.sum(0)
    mean = s[0] / M
    var = torch.clamp(s[1] / M - mean * mean, min=0.0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def sums_from_part(part, dgamma0=None, dbeta0=None):
    """part [rows][2][C] = per-row sums of g' and g' * xhat -> (dgamma, dbeta) as pesr_bn_lrelu_bwd_fused must make them; with dgamma0 /
    dbeta0 the accumulate form."""
    s = part.sum(0)
    dbeta, dgamma = s[0], s[1]
    if dgamma0 is not None:
        dgamma, dbeta = dgamma0 + dgamma, dbeta0 + dbeta
    return dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def act(z, slope):
    """slope 0.2: LeakyReLU, 0: ReLU, 1: none.  Whatever is not > 0 takes the slope: +0.0 and -0.0 do."""
    return torch.where(z > 0, z, z * slope)


def act_grad(z, dy, slope):
    """dz = dy * act'(z), with the same `> 0`."""
    return torch.where(z > 0, dy, dy * slope)


def normalize(x, mean, invstd):
    return (x - mean) * invstd


def pre_activation(x, gamma, beta, mean, invstd):
    """z = gamma * xhat + beta"""
    return gamma * normalize(x, mean, invstd) + beta


def apply(x, gamma, beta, mean, invstd, slope, y_nchw=False):
    """y = act(gamma * (x - mean) * invstd + beta), NHWC or NCHW"""
    y = act(pre_activation(x, gamma, beta, mean, invstd), slope)
    return y.permute(0, 3, 1, 2).contiguous() if y_nchw else y


def train_forward(x, gamma, beta, eps, slope, y_nchw=False):
    """-> (y, mean, var, invstd) from the batch's own statistics"""
    mean, var, invstd = batch_stats(x, eps)
    return apply(x, gamma, beta, mean, invstd, slope, y_nchw), mean, var, invstd


# ------------------------------------------------------------------------------------------------
# backward (dy: gradient at the activation's output, NHWC)
# ------------------------------------------------------------------------------------------------
def backward(x, dy, gamma, beta, mean, invstd, slope, training=True, dgamma0=None, dbeta0=None):
    """-> (dx, dgamma, dbeta).  dz = dy * act'(z); dbeta = sum dz, dgamma = sum dz * xhat;
    training: dx = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)); eval (fixed statistics): dx = gamma * invstd * dz.
    dgamma0 / dbeta0: the accumulate form adds to them."""
    xhat = normalize(x, mean, invstd)
    dz = act_grad(gamma * xhat + beta, dy, slope)
    return backward_masked(xhat, dz, gamma, invstd, training, dgamma0, dbeta0)


def backward_masked(xhat, dz, gamma, invstd, training=True, dgamma0=None, dbeta0=None):
    """The same from xhat and the already masked gradient dz."""
    dbeta, dgamma = dz.sum(ROWS), (dz * xhat).sum(ROWS)
    if training:
        M = rows(xhat)
        dx = gamma * invstd * (dz - dbeta / M - xhat * (dgamma / M))
    else:
        dx = gamma * invstd * dz
    if dgamma0 is not None:
        dgamma, dbeta = dgamma0 + dgamma, dbeta0 + dbeta
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------
# backward of the training backward: dz = gamma * s * (du - mean(du) - xhat * mean(du * xhat)), s = invstd, and g = dL/d(dz)
# ------------------------------------------------------------------------------------------------
def bwd_bwd_means(z, du, g, mean, invstd):
    """-> xhat and the channel means (m1, m2, G1, Gx, Ga) = mean of (du, du xhat, g, g xhat, g (du - m1))"""
    xhat = normalize(z, mean, invstd)
    m1 = du.mean(ROWS)
    return xhat, m1, (du * xhat).mean(ROWS), g.mean(ROWS), (g * xhat).mean(ROWS), (g * (du - m1)).mean(ROWS)


def bwd_bwd(z, du, g, gamma, mean, invstd):
    """-> (L_du, L_z, L_gamma), the closed forms of bn.hip's header:
        L_du    = gamma s (g - G1 - xhat Gx)
        L_z     = -gamma s^2 [xhat (Ga - 3 m2 Gx) + m2 (g - G1) + Gx (du - m1)]
        L_gamma = s M (Ga - m2 Gx)        (= s (sum(g du) - m1 sum(g) - m2 sum(g xhat)))
    tests/test_bn_cpu.py holds them against autograd through the first-order formula."""
    xhat, m1, m2, G1, Gx, Ga = bwd_bwd_means(z, du, g, mean, invstd)
    l_du = gamma * invstd * (g - G1 - xhat * Gx)
    l_z = -gamma * invstd * invstd * (xhat * (Ga - 3.0 * m2 * Gx) + m2 * (g - G1) + Gx * (du - m1))
    l_gamma = invstd * rows(z) * (Ga - m2 * Gx)
    return l_du, l_z, l_gamma
