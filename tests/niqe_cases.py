"""Inputs shared by the NIQE tests (tests/test_niqe_gpu.py, tests/golden/make_golden_niqe.py): the shapes, the seeded images, the
restatement's results for them (computed once per process) and the fixed model the scores are taken against."""
import functools

import numpy as np

import niqe_oracle as NO

# (H, W, B, shave, N)
SHAPES = [
    (8, 16, 8, 0, 1),          # the smallest legal case: two blocks, scale-2 blocks of 4
    (24, 48, 24, 0, 1),
    (50, 77, 24, 1, 1),        # crop tails on both axes
    (96, 192, 96, 0, 1),       # the real block size, twice
    (100, 131, 16, 4, 3),      # both layouts, and mixed
]
KINDS = ("u8", "float")
LUMAS = ("gray", "y")

# A fixed, well-conditioned model for the score checks: plausible feature means, a diagonal covariance.  (Any mean and any positive
# definite covariance make a model; this one keeps the pseudo-inverse far from a rank decision, so that a score's sensitivity to the
# block sums is that of the features and not of a threshold.)
MODEL_MU = np.tile(np.array([2.5, 0.7] + [0.8, 0.0, 0.5, 0.5] * 4), 2)
MODEL_COV = 0.04 * np.eye(36)


def seed_of(h, w, B, shave, n, kind, luma):
    return 4000 + h + 7 * w + 13 * B + shave + n + (100 if kind == "float" else 0) + (1000 if luma == "y" else 0)


def images(kind, n, h, w, seed):
    """[n, 3, h, w] float32.  u8: a smooth ramp plus blocky edges plus noise, rounded to 0..255.  float: what a Generator puts out:
    the same scaled to non-integer values in about -20 .. 280."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = rng.integers(40, 216, (n, 3, (h + 5) // 6, (w + 5) // 6)).astype(np.float64)
    a = np.kron(base, np.ones((6, 6)))[:, :, :h, :w] * 0.5 + (yy * 1.3 + xx * 0.9)[None, None] + rng.normal(0.0, 9.0, (n, 3, h, w))
    if kind == "u8":
        a = np.clip(np.rint(a), 0, 255)
    else:
        a = a * (300.0 / 255.0) - 20.0 + rng.uniform(-0.5, 0.5, a.shape)
    return a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(h, w, B, shave, n, kind, luma):
    """-> (images [n,3,h,w] float32, per image: dict of the restatement's stats, maps, features, alpha indices, smallest gap, score or
    None when fewer than two blocks have finite features).  Computed once; treat as read-only."""
    a = images(kind, n, h, w, seed_of(h, w, B, shave, n, kind, luma))
    a.setflags(write=False)
    out = []
    for i in range(n):
        st, m1, m2 = NO.stats(a[i], shave, B, luma)
        feat, index, gap = NO.features(st, B)
        try:
            sc = NO.score(feat, MODEL_MU, MODEL_COV)
        except ValueError:
            sc = None
        out.append({"stats": st, "m1": m1, "m2": m2, "feat": feat, "index": index, "gap": gap, "score": sc})
    return a, out


def perturbed_score_change(res, B, draws=20, seed=0):
    """The largest relative change of the restatement's score when every sum of its stats is moved by a random sign times
    (n - 1) * 2^-53 relative (n the block's pixel count at that scale): what a reduction in another order may do."""
    if res["score"] is None:
        return 0.0
    rng = np.random.default_rng(seed)
    worst = 0.0
    sums = [j for j in range(26) if j % 5 not in (1, 3) or j == 25]
    for _ in range(draws):
        st = res["stats"].copy()
        for sc in range(2):
            npix = (B >> sc) * (B >> sc)
            sign = rng.choice([-1.0, 1.0], size=(st.shape[1], len(sums)))
            st[sc][:, sums] = st[sc][:, sums] * (1.0 + sign * (npix - 1) * 2.0 ** -53)
        feat, _, _ = NO.features(st, B)
        worst = max(worst, abs(NO.score(feat, MODEL_MU, MODEL_COV) - res["score"]) / res["score"])
    return worst
