"""Writes gv15_degrade.npz: small uint8 images, their blur kernels and the outputs of tests/degrade_oracle.py (the float64
restatement of docs/modes.md section 4j) - so that a later edit of the restatement cannot move the definition unnoticed.
Case n: image `in<n>`, kernel `k<n>`, `par<n>` = (s, sigma_n, q, y0, x0, h, w) as float64 (q below 2^53), output `out<n>`.
Run from the repository root: python tests/golden/make_golden_degrade.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import degrade_oracle as D  # noqa: E402


def cases():
    rng = np.random.default_rng(20241017)
    y, x = np.mgrid[0:24, 0:36]
    ramp = np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (5 * x + 2 * y) // 2 % 256], axis=2).astype(np.uint8)
    rand = rng.integers(0, 256, (24, 36, 3), dtype=np.uint8)
    box = lambda K: np.full((K, K), 1.0 / (K * K))
    # (image, s, kernel, sigma_n, q, window or None)
    return [(ramp, 2, box(2), 0.0, 0, None),
            (ramp, 4, box(4), 0.0, 0, None),
            (rand, 3, D.gaussian_kernel(11, 1.6), 0.0, 0, None),
            (rand, 2, D.gaussian_kernel(10, 1.6, 0.5, 0.6), 12.5, 77, None),
            (rand, 4, D.gaussian_kernel(24, 3.2, 1.1, 2.2), 30.0, 1234567, (1, 2, 4, 6)),
            (rand, 3, D.gaussian_kernel(23, 2.4), 0.0, 0, (7, 11, 1, 1)),
            (np.zeros((6, 6, 3), np.uint8), 3, box(1), 30.0, 5, None)]


def main():
    out = {}
    for n, (img, s, k, sigma_n, q, win) in enumerate(cases()):
        y0, x0, h, w = win if win is not None else (0, 0, img.shape[0] // s, img.shape[1] // s)
        out[f"in{n}"], out[f"k{n}"] = img, k
        out[f"par{n}"] = np.array([s, sigma_n, q, y0, x0, h, w], dtype=np.float64)
        out[f"out{n}"] = D.degrade(img, s, k, sigma_n, q, (y0, x0, h, w))
    np.savez_compressed(os.path.join(HERE, "gv15_degrade.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
