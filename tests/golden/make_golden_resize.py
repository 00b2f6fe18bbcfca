"""Writes gv14_imresize.npz: small uint8 images and the outputs of tests/resize_oracle.py (the float64 restatement of
docs/modes.md section 4f) at s = 2, 3, 4, down and up - so that a later edit of the restatement cannot move the definition
unnoticed.  Down-resizes take the mod-cropped image.  Run from the repository root: python tests/golden/make_golden_resize.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_oracle as R  # noqa: E402


def images():
    rng = np.random.default_rng(20181014)
    y, x = np.mgrid[0:18, 0:24]
    ramp = np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (5 * x + 2 * y) // 2 % 256], axis=2).astype(np.uint8)
    return {"random": rng.integers(0, 256, (12, 18, 3), dtype=np.uint8),
            "ramp": ramp,
            "ragged": rng.integers(0, 256, (17, 14, 3), dtype=np.uint8)}


def main():
    out = {}
    for name, img in images().items():
        out[f"{name}_in"] = img
        for s in (2, 3, 4):
            out[f"{name}_down{s}"] = R.imresize(R.modcrop(img, s), s, up=False)
            out[f"{name}_up{s}"] = R.imresize(img, s, up=True)
    np.savez_compressed(os.path.join(HERE, "gv14_imresize.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
