"""CPU: the bf16 family's four tile planners (conv3x3_bf16.hip b16_plan / b16_plan_s2 / b16_plan_s2d, conv3x3_bf16x3.hip b3_plan,
which share one tile search in conv3x3_bf16_common.h) against a recording of the four separate searches they replaced
(tests/golden/bf16_plan_scores.json, written by tests/golden/make_golden_bf16_plans.py at the commit before the shared search): every
recorded integer, not only which side of the dispatch threshold it is on.  Needs the built library for the host-only score entry
points, no GPU."""
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_plan_scores.json")
KEYS = ("N", "H", "W", "Cin", "Cout", "min_wgs")
SIZES = [1, 2, 5, 7, 11, 12, 13, 24, 47, 48, 96, 144, 145, 192]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["points"] = list(itertools.product(*(g["grid"][k] for k in KEYS)))
    # the file keeps each distinct block of len(Cout) * len(min_wgs) scores once, and per (N, H, W, Cin) in grid order the block's number
    g["scores"] = {fn: [s for i in rec["index"] for s in rec["blocks"][i]] for fn, rec in g["scores"].items()}
    return g


def test_recording_is_the_grid_it_says(golden):
    assert golden["functions"] == ["pesr_conv3x3_bf16_score", "pesr_conv3x3_bf16_s2_score", "pesr_conv3x3_bf16_s2_dgrad_score",
                                   "pesr_conv3x3_bf16x3_score"]
    assert golden["grid"] == {"N": [1, 2, 16], "H": SIZES, "W": SIZES, "Cin": [32, 64, 96, 256], "Cout": [64, 96, 128, 256, 512, 1024],
                              "min_wgs": [1, 64, 128]}
    assert len(golden["points"]) == 3 * 14 * 14 * 4 * 6 * 3
    for fn in golden["functions"]:
        scores = golden["scores"][fn]
        assert len(scores) == len(golden["points"])
        assert all(isinstance(s, int) and 0 <= s <= 1000 for s in scores)
        assert any(s > 0 for s in scores) and any(s == 0 for s in scores), fn      # non-zero somewhere, zero somewhere


@pytest.mark.parametrize("fn", ["pesr_conv3x3_bf16_score", "pesr_conv3x3_bf16_s2_score", "pesr_conv3x3_bf16_s2_dgrad_score",
                                "pesr_conv3x3_bf16x3_score"])
def test_planner_reproduces_every_recorded_score(golden, fn):
    from pesr_amd import _lib
    f = getattr(_lib.lib(), fn)
    got = [int(f(*p)) for p in golden["points"]]
    assert any(s > 0 for s in got) and any(s == 0 for s in got)
    bad = [(p, w, g) for p, w, g in zip(golden["points"], golden["scores"][fn], got) if w != g]
    assert not bad, f"{fn}: {len(bad)} of {len(got)} scores differ from the recording, first (point, recorded, got): {bad[:5]}"
