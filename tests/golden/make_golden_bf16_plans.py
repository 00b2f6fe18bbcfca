"""Writes bf16_plan_scores.json: the integer answers of the bf16 family's four tile planners (the host-only score entry points
pesr_conv3x3_bf16_score, pesr_conv3x3_bf16_s2_score, pesr_conv3x3_bf16_s2_dgrad_score, pesr_conv3x3_bf16x3_score) over a grid of
problems, as computed by the commit this script is run at - the commit BEFORE the four planners shared one tile search
(conv3x3_bf16_common.h).  The file holds every integer of the grid, distinct blocks written once (encode below);
tests/test_bf16_plans_cpu.py holds the library to every one of them.  Needs the built library, no
GPU.  Run from the repository root: python tests/golden/make_golden_bf16_plans.py
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pesr_amd import _lib  # noqa: E402

FUNCTIONS = ["pesr_conv3x3_bf16_score", "pesr_conv3x3_bf16_s2_score", "pesr_conv3x3_bf16_s2_dgrad_score", "pesr_conv3x3_bf16x3_score"]
SIZES = [1, 2, 5, 7, 11, 12, 13, 24, 47, 48, 96, 144, 145, 192]
GRID = {"N": [1, 2, 16],
        "H": SIZES,
        "W": SIZES,
        "Cin": [32, 64, 96, 256],
        "Cout": [64, 96, 128, 256, 512, 1024],
        "min_wgs": [1, 64, 128]}
KEYS = ("N", "H", "W", "Cin", "Cout", "min_wgs")


def points(grid=GRID):
    """The grid in file order: itertools.product over the keys as listed, the last one fastest."""
    return itertools.product(*(grid[k] for k in KEYS))


def encode(scores):
    """The scores of one function in file order -> (blocks, index).  A block is the len(Cout) * len(min_wgs) scores of one (N, H, W, Cin);
    the file keeps each distinct block once and, per (N, H, W, Cin) in file order, its number: every integer of the grid, in a
    fraction of the bytes (the scores depend on Cin only through the argument checks)."""
    n = len(GRID["Cout"]) * len(GRID["min_wgs"])
    blocks, index = [], []
    for i in range(0, len(scores), n):
        b = scores[i:i + n]
        if b not in blocks:
            blocks.append(b)
        index.append(blocks.index(b))
    return blocks, index


def decode(blocks, index):
    return [s for i in index for s in blocks[i]]


def main():
    lib = _lib.lib()
    out = {}
    for fn in FUNCTIONS:
        f = getattr(lib, fn)
        scores = [int(f(*p)) for p in points()]
        assert any(scores) and not all(scores), f"{fn} is constant over the grid: widen it"
        blocks, index = encode(scores)
        assert decode(blocks, index) == scores
        out[fn] = {"blocks": blocks, "index": index}
    path = os.path.join(HERE, "bf16_plan_scores.json")
    per_line = len(GRID["W"]) * len(GRID["Cin"])                # one line of block numbers per (N, H)
    with open(path, "w") as f:
        f.write('{"functions":%s,\n"grid":%s,\n"scores":{\n' % (json.dumps(FUNCTIONS, separators=(",", ":")), json.dumps(GRID, separators=(",", ":"))))
        for k, fn in enumerate(FUNCTIONS):
            b, ix = out[fn]["blocks"], out[fn]["index"]
            f.write('"%s":{"blocks":[\n%s],\n"index":[\n%s]}%s\n' % (
                fn, ",\n".join(",".join(json.dumps(x, separators=(",", ":")) for x in b[i:i + 4]) for i in range(0, len(b), 4)),
                ",\n".join(",".join(map(str, ix[i:i + per_line])) for i in range(0, len(ix), per_line)), "," if k + 1 < len(FUNCTIONS) else ""))
        f.write("}}\n")
    with open(path) as f:                                       # what was written is JSON and holds every score
        back = json.load(f)
    assert all(len(decode(**back["scores"][fn])) == len(list(points())) for fn in FUNCTIONS)
    print({fn: (len(v["index"]), len(v["blocks"])) for fn, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
