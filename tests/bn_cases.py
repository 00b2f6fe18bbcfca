"""Inputs and the rounding-error model shared by tests/test_bn_cpu.py and tests/test_bn_gpu.py (docs/experiments/bn_tests.md).
TEST INFRASTRUCTURE; no GPU import."""
import numpy as np
import torch

import bn_oracle as BO
from oracle import detrand

U = 2.0 ** -24        # one fp32 rounding
D = 2.0 ** -40        # far above what the kernels' double-precision sums (rpb + nb <= 4624 additions at 2^-53 = 5e-13) can lose


def k(n):
    """n fp32 roundings in a row."""
    return (1.0 + U) ** n - 1.0


def f32(v):
    """A Python float as the C ABI's `float` argument receives it."""
    return float(np.float32(v))


EPS, SLOPE = f32(1e-5), f32(0.2)

# (mean, std) per channel of the conditioning case; r = |mean| / std.  Channel 6 is constant (var = 0: eps decides everything), channel 7
# has var = 1e-6 < eps.
COND = [(0.5, 1.44), (10.0, 1.0), (30.0, 1.0), (100.0, 1.0), (127.5, 0.5), (50.0, 0.05), (1000.1, 0.0), (0.0, 1e-3)]
COND_SHAPE = (2, 37, 50)
COND_FINITE_R = [0, 1, 2, 3, 4, 5]        # channels with 0 < r < inf (bn_bwd_bwd's cases are the five with r >= 10, and channel 0)


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def channels(shape, pairs, seed):
    """fp32 [N, H, W, C], channel c normal with pairs[c] = (mean, std)"""
    n = randn(tuple(shape) + (len(pairs),), seed).double()
    mean = torch.tensor([p[0] for p in pairs], dtype=torch.float64)
    std = torch.tensor([p[1] for p in pairs], dtype=torch.float64)
    return (mean + std * n).float()


def conditioning_input(seed=11):
    return channels(COND_SHAPE, COND, seed)


def affine(C, seed):
    """gamma in [0.5, 1.5], beta in [-0.3, 0.3]"""
    return detrand.uniform((C,), seed, 0.5, 1.5), detrand.uniform((C,), seed + 1, -0.3, 0.3)


def z_bound(x, gamma, beta, mean, invstd):
    """Bound on |z_fp32 - z_float64| for z = gamma * ((x - mean) * invstd) + beta evaluated in fp32 on the SAME fp32 operands: three
    roundings on the way to gamma * xhat, and the sum's own u |z| <= u (|gamma xhat| + |beta|).  An FMA rounds once less."""
    return k(4) * ((gamma * BO.normalize(x, mean, invstd)).abs() + beta.abs())


def ambiguous(x, gamma, beta, mean, invstd):
    """The set A: elements where fp32 and float64 may disagree on `z > 0` - |z| within the forward bound.  Where the bound is 0 (gamma
    xhat = 0 and beta = 0 exactly) z is 0 in both and nothing is ambiguous."""
    b = z_bound(x, gamma, beta, mean, invstd)
    return (BO.pre_activation(x, gamma, beta, mean, invstd).abs() <= b) & (b > 0)


AMBIGUOUS_CAP = 1e-3
