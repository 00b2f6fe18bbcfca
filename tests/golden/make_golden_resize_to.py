"""Makes tests/golden/gv18_resize_to.npz: outputs of the restatement tests/resize_to_oracle.py of docs/modes.md section 4m on one small
synthetic colour image (smooth gradients, a disc, a hard edge, fine noise), so that an edit of the restatement cannot move the
definition unnoticed.  Data produced by the restatement; the test reads the file only.

    python tests/golden/make_golden_resize_to.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_to_oracle as RT  # noqa: E402

SIZES = ((13, 97), (5, 7), (64, 31), (37, 53))
NOISE = (4.5, 20240229)                    # (sigma_n, stream) of the "noisy" outputs
JITTER = (0.37, 1.6)


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 170 * x / w, 60 + 120 * y / h, 200 - 150 * (x + y) / (h + w)], axis=2)
    disc = (y - 0.35 * h) ** 2 + (x - 0.3 * w) ** 2 < (0.2 * min(h, w)) ** 2
    img[disc] = (255, 190, 0)
    img[:, int(0.7 * w):] = (0, 70, 255)
    img[int(0.6 * h):, :int(0.4 * w)] += rng.normal(0, 25, (h - int(0.6 * h), int(0.4 * w), 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    img = image(37, 53, 3)
    out = {"src": img, "sizes": np.array(SIZES), "noise": np.array(NOISE), "jitter": np.array(JITTER)}
    for m in RT.METHODS:
        for ho, wo in SIZES:
            out[f"{m}_{ho}x{wo}"] = RT.resize(img, (ho, wo), m)
        out[f"{m}_noisy"] = RT.resize(img, SIZES[0], m, NOISE[0], int(NOISE[1]))
    for r in JITTER:
        for m1 in range(3):
            out[f"jitter_{r}_{m1}"] = RT.jitter(img, r, m1, (m1 + 1) % 3, NOISE[0], int(NOISE[1]))
    path = os.path.join(HERE, "gv18_resize_to.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
