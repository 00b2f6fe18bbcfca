"""Writes gv16_niqe.npz: three small images and what tests/niqe_oracle.py (the float64 restatement of docs/modes.md section 4k)
gives for them - block sums, features, alpha grid indices and the score against the fixed model of tests/niqe_cases.py - so that a
later edit of the restatement cannot move the definition unnoticed.
Case n: image `in<n>` [3, H, W], `par<n>` = (shave, B, luma: 0 gray / 1 y), `stats<n>`, `feat<n>`, `index<n>`, `score<n>`.
Run from the repository root: python tests/golden/make_golden_niqe.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import niqe_cases as C  # noqa: E402
import niqe_oracle as NO  # noqa: E402


def cases():
    # (image, shave, B, luma)
    return [(C.images("u8", 1, 30, 44, 161)[0].astype(np.uint8), 1, 8, "gray"),
            (C.images("float", 1, 24, 48, 162)[0], 0, 24, "y"),
            (C.images("u8", 1, 40, 56, 163)[0].astype(np.uint8), 4, 16, "gray")]


def main():
    out = {"count": np.int64(len(cases()))}
    for n, (img, shave, B, luma) in enumerate(cases()):
        st, _, _ = NO.stats(img, shave, B, luma)
        feat, index, gap = NO.features(st, B)
        out[f"in{n}"], out[f"par{n}"] = img, np.array([shave, B, 1 if luma == "y" else 0], dtype=np.int64)
        out[f"stats{n}"], out[f"feat{n}"], out[f"index{n}"] = st, feat, index
        out[f"score{n}"] = np.float64(NO.score(feat, C.MODEL_MU, C.MODEL_COV))
        print(n, img.shape, img.dtype, "finite rows", int(np.isfinite(feat).all(axis=1).sum()), "of", len(feat), "gap", gap, "score", out[f"score{n}"])
    np.savez_compressed(os.path.join(HERE, "gv16_niqe.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "gv16_niqe.npz")), "bytes")


if __name__ == "__main__":
    main()
