"""The cases of tests/test_dists_cpu.py and tests/test_dists_gpu.py, and their restated answers (computed once per process)."""
import functools
import warnings

import numpy as np

import dists_oracle as DO

# ---- the L2 pooling: (N, H, W, C) ---------------------------------------------------------------------------------------------------
# 2 x 2; 5 x 7, odd on both axes, where the last window reaches the padding; 1 x 1; C = 512; 11 x 13 at C = 64, 42 output pixels per
# image where a workgroup writes 16 (asserted from ops.l2pool_plan on the GPU)
L2POOL_CASES = ((2, 2, 2, 64), (2, 5, 7, 64), (2, 1, 1, 64), (2, 3, 2, 512), (2, 11, 13, 64))
L2POOL_BIG = (2, 11, 13, 64)


@functools.lru_cache(maxsize=None)
def l2pool_case(n, h, w, c):
    """-> (x [n,h,w,c] float32, post-ReLU-like with exact zeros; l2pool_f64(x))."""
    rng = np.random.default_rng([11, n, h, w, c])
    x = np.abs(rng.standard_normal((n, h, w, c)))
    x = np.where(rng.random(x.shape) < 0.3, 0.0, x).astype(np.float32)
    x.setflags(write=False)
    return x, DO.l2pool_f64(x)


# ---- the head: (C, (H, W)) at N = 2 -------------------------------------------------------------------------------------------------
# P = 1; P = 35; P = 257, the smallest that takes two pixel blocks; P = 573 = 2 blocks and a tail of 61 (ops.dists_plan asserted on the GPU)
LAYER_N = 2
LAYER_CHANNELS = (3, 64, 512)
LAYER_SIZES = ((1, 1), (5, 7), (1, 257), (3, 191))
# "relu": post-ReLU-like; "mean": mean 1e3, spread 1e-2, where an uncentred form loses digits; "zero": a channel of exact zeros in both maps
KINDS = ("relu", "mean", "zero")
LAYER_CASES = [(c, hw) for c in LAYER_CHANNELS for hw in LAYER_SIZES]


@functools.lru_cache(maxsize=None)
def layer_case(c, hw, kind):
    """-> (fa, fb [2,h,w,c] float32, alpha, beta [c] float64: a slice's worth of normalised weights)."""
    h, w = hw
    rng = np.random.default_rng([13, c, h, w, KINDS.index(kind)])
    shape = (LAYER_N, h, w, c)
    if kind == "mean":
        fa = (1e3 + 1e-2 * rng.standard_normal(shape)).astype(np.float32)
        fb = (1e3 + 1e-2 * rng.standard_normal(shape)).astype(np.float32)
    else:
        fa = np.abs(rng.standard_normal(shape))
        fa = np.where(rng.random(shape) < 0.5, 0.0, fa).astype(np.float32)
        fb = (fa + 0.3 * np.abs(rng.standard_normal(shape))).astype(np.float32)
        fb[1] = np.where(rng.random(shape[1:]) < 0.5, 0.0, np.abs(rng.standard_normal(shape[1:]))).astype(np.float32)      # pair 1: unrelated
    if kind == "zero":
        fa[..., c - 1] = 0.0                                        # channel C - 1: the last lane's
        fb[..., c - 1] = 0.0
    alpha = (0.1 + 0.01 * rng.standard_normal(c)) / 295.0
    beta = (0.1 + 0.01 * rng.standard_normal(c)) / 295.0
    for t in (fa, fb, alpha, beta):
        t.setflags(write=False)
    return fa, fb, alpha, beta


@functools.lru_cache(maxsize=None)
def layer_ordered(c, hw, kind):
    """-> (contribution [2], statistics [2, c, 5])."""
    return DO.layer_ordered(*layer_case(c, hw, kind))


# ---- the whole metric --------------------------------------------------------------------------------------------------------------
MODEL_SEED = 9
# (the shape that is scored, shave): with shave 2 the image is 4 larger on both sides, so that what the trunk sees is the same
# 16 x 16 (one pixel after the four pools), 17 x 23 (odd sides at every pool) and 33 x 19
METRIC_SHAPES = ((2, 3, 16, 16), (2, 3, 17, 23), (1, 3, 33, 19))
METRIC_CASES = tuple((s, shave) for s in METRIC_SHAPES for shave in (0, 2))
# The largest absolute difference between dists_trunk32 (a float32 trunk of direct convs on the CPU, every sum in one stated order, so
# the figure is the same on every machine) and dists_f64 over TRUNK32_CASES (METRIC_CASES and one 48 x 48 pair), measured by
# tests/test_dists_cpu.py::test_float32_trunk_against_float64, which asserts that the measurement does not exceed this: 5.859e-08, at
# (2, 3, 16, 16) shave 2, the unrelated pair (score 0.188); 3.1e-06 of the score at the worst, a noisy copy (score 0.0032).  The
# tolerance is absolute, because the score is one minus a sum near one.  The device adds the rounding of the Winograd F(4,3) transforms,
# which these cases sample and do not bound: the GPU tolerance is 16 times this, 9.374e-07.
TRUNK32_CASES = METRIC_CASES + (((1, 3, 48, 48), 0),)
TRUNK32_ABS = 5.859e-8
SCORE_ATOL = 16 * TRUNK32_ABS


@functools.lru_cache(maxsize=None)
def model():
    from pesr_amd.dists import DistsModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DistsModel.random(MODEL_SEED)


@functools.lru_cache(maxsize=None)
def model_tensors():
    return model().tensors()


@functools.lru_cache(maxsize=None)
def image_pair(shape, shave=0):
    """Two images [n,3,h + 2 shave,w + 2 shave] of integer values 0..255 as float32: pair 0 (the only one at n = 1 and shave 0) is
    smooth blocks plus noise and a noisy copy of it; the last pair at n = 2, and the pair at n = 1 with a shave, are unrelated images."""
    n, _, h, w = shape
    h, w = h + 2 * shave, w + 2 * shave
    rng = np.random.default_rng([17, n, h, w])

    def blocks():
        base = np.kron(rng.integers(20, 236, (n, 3, -(-h // 8), -(-w // 8))), np.ones((8, 8)))[:, :, :h, :w]
        return np.clip(np.rint(base + rng.normal(0, 8, (n, 3, h, w))), 0, 255).astype(np.float32)
    a = blocks()
    b = np.clip(np.rint(a + rng.normal(0, 12, (n, 3, h, w))), 0, 255).astype(np.float32)
    other = blocks()
    if n > 1 or shave:
        b[n - 1] = other[n - 1]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def metric_f64(shape, shave):
    """-> (score [n], the six stage contributions [6, n])."""
    a, b = image_pair(shape, shave)
    return DO.dists_f64(a, b, model_tensors(), shave, return_parts=True)


@functools.lru_cache(maxsize=None)
def metric_trunk32(shape, shave):
    a, b = image_pair(shape, shave)
    return DO.dists_trunk32(a, b, model_tensors(), shave)
