"""The cases of tests/test_lpips_loss_cpu.py and tests/test_lpips_loss_gpu.py for the head's gradient, and their restated answers
(computed once per process)."""
import functools

import numpy as np

import lpips_cases as C
import lpips_grad_oracle as GO

CHANNELS = C.CHANNELS
# 1, 15, 16, 17, 64 and 65 pixels: one pixel, the unroll tail, exactly one wave, the wave tail, exactly one workgroup, a second one
SHAPES = ((1, 1), (3, 5), (4, 4), (1, 17), (8, 8), (5, 13))
BATCHES = (1, 2)
# relu: post-ReLU-like features;  zeros: all-zero pixels in a, in b, in both;  same: b = a;  near: b = a (1 + 1e-4 noise), t cancels;
# wzeros: half of the weights zero
KINDS = ("relu", "zeros", "same", "near", "wzeros")
CASES = [(c, n, h, w) for c in CHANNELS for (h, w) in SHAPES for n in BATCHES]
SPECIAL = [(c, 2, 5, 13) for c in CHANNELS] + [(64, 1, 1, 1), (512, 1, 3, 5)]      # the shapes the other kinds run at


@functools.lru_cache(maxsize=None)
def case(c, n, h, w, kind):
    """-> (fa, fb [n,h,w,c] float32, weights [c] float32, g [n] float64 with a value of its own per image)."""
    rng = np.random.default_rng([41, c, n, h, w, KINDS.index(kind)])
    shape = (n, h, w, c)
    fa, fb = C._relu_like(rng, shape), C._relu_like(rng, shape)
    wt = rng.random(c).astype(np.float32)
    g = (rng.standard_normal(n) + 3.0 * (np.arange(n) - 0.25)).astype(np.float64)
    if kind == "zeros":
        pick = rng.integers(0, 4, (n, h, w))                        # 0: a zero, 1: b zero, 2: both, 3: neither
        if pick.size >= 3:
            pick.reshape(-1)[:3] = (0, 1, 2)
        else:
            pick[...] = 0
        fa[(pick == 0) | (pick == 2)] = 0.0
        fb[(pick == 1) | (pick == 2)] = 0.0
    elif kind == "same":
        fb = fa.copy()
    elif kind == "near":
        fb = (fa.astype(np.float64) * (1.0 + 1e-4 * rng.standard_normal(shape))).astype(np.float32)
    elif kind == "wzeros":
        wt[rng.random(c) < 0.5] = 0.0
        wt[0] = 0.0
    for t in (fa, fb, wt, g):
        t.setflags(write=False)
    return fa, fb, wt, g


@functools.lru_cache(maxsize=None)
def ordered(c, n, h, w, kind):
    return GO.grad_ordered(*case(c, n, h, w, kind))


@functools.lru_cache(maxsize=None)
def exact_and_bound(c, n, h, w, kind):
    args = case(c, n, h, w, kind)
    return GO.grad_exact(*args), GO.grad_bound(*args)
