"""The inputs of the SSIM-loss tests (docs/modes.md section 4p) and their restated results, each computed once and shared."""
import functools

import numpy as np

import ssim_loss_oracle as O

KINDS = ("noise", "same", "const", "const_noise")

# H x W.  The forward tiles the (H-10) x (W-10) map in 16 x 32, the backward the H x W image in 16 x 32.
SHAPES = [
    (11, 11),            # a single window
    (11, 58), (26, 11),  # one row / one column of windows
    (13, 15),            # a 3 x 5 map: smaller than the backward's halo of 10 in both directions
    (16, 32), (17, 32), (16, 33),     # exactly one backward tile, and one past it in each direction
    (26, 42), (27, 42), (26, 43),     # exactly one forward tile (a 16 x 32 map), and one past it in each direction
    (47, 80),            # 3 x 3 tiles with tails in both directions, for both kernels (map 37 x 70)
]
BATCHES = (1, 3)


@functools.lru_cache(maxsize=None)
def case(kind, n, h, w):
    """-> (a, b, g): a = sr and b = hr [n, 3, h, w] float32, g float64 [n], distinct per image.  Read-only arrays."""
    rng = np.random.default_rng([KINDS.index(kind), n, h, w])
    hr = rng.integers(0, 256, (n, 3, h, w)).astype(np.float32)
    noisy = (hr + rng.normal(0.0, 25.0, hr.shape)).astype(np.float32)       # a generator's output: not integer, not inside 0 .. 255
    if kind == "noise":
        a, b = noisy, hr
    elif kind == "same":
        a, b = noisy, noisy.copy()
    elif kind == "const":
        a, b = np.full_like(hr, 100.0), np.full_like(hr, 103.0)
    else:
        a, b = np.full_like(hr, 77.0), hr
    g = (rng.uniform(0.5, 1.5, n) * np.where(np.arange(n) % 2, -1.0, 1.0)).astype(np.float64)
    for t in (a, b, g):
        t.setflags(write=False)
    return a, b, g


@functools.lru_cache(maxsize=None)
def ordered(kind, n, h, w):
    """-> (score [n], coef [n, 3, h-10, w-10], grad float32 [n, 3, h, w]) of the restatement."""
    a, b, g = case(kind, n, h, w)
    out = (O.score_ordered(a, b), O.coef_ordered(a, b), O.grad_ordered(a, b, g))
    for t in out:
        t.setflags(write=False)
    return out
