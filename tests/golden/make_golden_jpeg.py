"""Makes tests/golden/gv17_jpeg.npz: the outside witness of docs/modes.md section 4l.  Two small synthetic colour images (smooth
regions, an edge, fine noise; one with odd sides, one a multiple of 16), what Pillow's libjpeg returns for them - decode(encode) at
the qualities 10, 50, 75, 90 and at their neighbours q - 15 and q + 15 (kept inside 1 .. 100), 4:4:4 and 4:2:0 - and what the
restatement tests/jpeg_oracle.py returns at the four qualities.  Data produced by a codec and by the restatement; the test reads the
file only, so it does not depend on the Pillow of the machine it runs on.

    python tests/golden/make_golden_jpeg.py        (needs Pillow with JPEG support)
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_oracle as JO  # noqa: E402

QUALITIES = (10, 50, 75, 90)
STEP = 15


def neighbours(q):
    return max(1, q - STEP), min(100, q + STEP)


def image(h, w, seed):
    """Smooth colour gradients, a bright disc on them, a hard vertical edge into a flat region, fine noise in one corner."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 170 * x / w, 60 + 120 * y / h, 200 - 150 * (x + y) / (h + w)], axis=2)
    disc = (y - 0.35 * h) ** 2 + (x - 0.3 * w) ** 2 < (0.2 * min(h, w)) ** 2
    img[disc] = (230, 190, 60)
    img[:, int(0.7 * w):] = (30, 70, 140)
    img[int(0.6 * h):, :int(0.4 * w)] += rng.normal(0, 25, (h - int(0.6 * h), int(0.4 * w), 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pillow_round_trip(img, q, chroma420):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=2 if chroma420 else 0)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))


def main():
    import PIL
    from PIL import features
    out = {"qualities": np.array(QUALITIES), "step": np.array(STEP),
           "versions": np.array([f"Pillow {PIL.__version__}", f"libjpeg{'-turbo' if features.check_feature('libjpeg_turbo') else ''} "
                                 f"{features.version('jpg')}"])}
    for name, (h, w, seed) in {"odd": (37, 53, 1), "mcu": (48, 64, 2)}.items():
        img = image(h, w, seed)
        out[f"{name}_src"] = img
        for mode, c420 in (("444", False), ("420", True)):
            for q in sorted({q for Q in QUALITIES for q in (Q,) + neighbours(Q)}):
                out[f"{name}_{mode}_pillow_q{q}"] = pillow_round_trip(img, q, c420)
            for q in QUALITIES:
                out[f"{name}_{mode}_ours_q{q}"] = JO.jpeg(img, q, c420)
    path = os.path.join(HERE, "gv17_jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
