"""The cases of tests/test_lpips_cpu.py and tests/test_lpips_gpu.py, and their restated answers (computed once per process)."""
import functools
import warnings

import numpy as np

import lpips_oracle as LO

CHANNELS = (64, 128, 256, 512)
HEAD_SHAPES = ((1, 1, 1), (2, 3, 5), (1, 2, 67), (3, 9, 7))
BIG_SHAPE = (2, 67, 129)                                            # C = 64 only: 136 workgroups per image, 3 pixels in the last
# (i) post-ReLU-like  (ii) with all-zero pixels in a, in b, in both  (iii) b = a  (iv) b = a (1 + 1e-6 noise)
# (v) w with zeros; one non-zero w_c, in the last lane's share
KINDS = ("relu", "zeros", "same", "near", "wzeros", "wone")
HEAD_CASES = [(C, n, h, w) for C in CHANNELS for (n, h, w) in HEAD_SHAPES] + [(64,) + BIG_SHAPE]


def _relu_like(rng, shape):
    x = np.abs(rng.standard_normal(shape))
    return np.where(rng.random(shape) < 0.5, 0.0, x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def head_case(C, n, h, w, kind):
    """-> (fa, fb [n,h,w,C] float32, weights [C] float32)."""
    rng = np.random.default_rng([C, n, h, w, KINDS.index(kind)])
    shape = (n, h, w, C)
    fa, fb = _relu_like(rng, shape), _relu_like(rng, shape)
    wt = rng.random(C).astype(np.float32)
    if kind == "zeros":
        pick = rng.integers(0, 4, (n, h, w))                       # 0: a zero, 1: b zero, 2: both, 3: neither
        if pick.size >= 3:
            pick.reshape(-1)[:3] = (0, 1, 2)
        else:
            pick[...] = 2
        fa[(pick == 0) | (pick == 2)] = 0.0
        fb[(pick == 1) | (pick == 2)] = 0.0
    elif kind == "same":
        fb = fa.copy()
    elif kind == "near":
        fb = (fa.astype(np.float64) * (1.0 + 1e-6 * rng.standard_normal(shape))).astype(np.float32)
    elif kind == "wzeros":
        wt[rng.random(C) < 0.5] = 0.0
    elif kind == "wone":
        wt[:] = 0.0
        wt[C - 1] = 0.75                                            # channel C - 1: lane 63's last
    for t in (fa, fb, wt):
        t.setflags(write=False)
    return fa, fb, wt


@functools.lru_cache(maxsize=None)
def head_answers(C, n, h, w, kind):
    """-> {"ordered": (score, map), "exact": (score, map), "bound": (score bound, map bound)}."""
    fa, fb, wt = head_case(C, n, h, w, kind)
    return {"ordered": LO.head_ordered(fa, fb, wt), "exact": LO.head_exact(fa, fb, wt), "bound": LO.head_bound(fa, fb, wt)}


# ---- the whole metric --------------------------------------------------------------------------------------------------------------
MODEL_SEED = 5
# shave 0 and 3 at every shape that survives it: 16 x 16 with shave 3 is 10 x 10, which lpips() refuses (tested as a refusal)
METRIC_CASES = (((1, 3, 16, 16), 0), ((2, 3, 37, 51), 0), ((2, 3, 37, 51), 3), ((1, 3, 64, 48), 0), ((1, 3, 64, 48), 3))
MIN_SCORE = 1e-3
# The largest relative difference between lpips_trunk32 (direct float32 convs on the CPU) and lpips_f64 over METRIC_CASES, measured by
# tests/test_lpips_cpu.py::test_float32_trunk_against_float64: 1.218e-07, at (1, 3, 16, 16) shave 0.  The device adds the rounding of
# the Winograd F(4,3) transforms, which these cases sample and do not bound: the tolerance is 16 times the measurement.
TRUNK32_REL = 1.218e-7
SCORE_RTOL = 16 * TRUNK32_REL


@functools.lru_cache(maxsize=None)
def model():
    from pesr_amd.lpips import LpipsModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LpipsModel.random(MODEL_SEED)


@functools.lru_cache(maxsize=None)
def model_tensors():
    return model().tensors()


@functools.lru_cache(maxsize=None)
def image_pair(shape):
    """Two images of integer values 0..255 as float32: smooth blocks plus noise, and a disturbed copy of it."""
    n, _, h, w = shape
    rng = np.random.default_rng([7, n, h, w])
    base = np.kron(rng.integers(20, 236, (n, 3, -(-h // 8), -(-w // 8))), np.ones((8, 8)))[:, :, :h, :w]
    a = np.clip(np.rint(base + rng.normal(0, 8, (n, 3, h, w))), 0, 255).astype(np.float32)
    b = np.clip(np.rint(a + rng.normal(0, 12, (n, 3, h, w))), 0, 255).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def metric_f64(shape, shave):
    a, b = image_pair(shape)
    return LO.lpips_f64(a, b, model_tensors(), shave)


@functools.lru_cache(maxsize=None)
def metric_trunk32(shape, shave):
    a, b = image_pair(shape)
    return LO.lpips_trunk32(a, b, model_tensors(), shave)
