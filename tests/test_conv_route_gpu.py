"""The routing of every 3x3 conv node of pesr_amd/functional.py (_conv_fwd, _conv_wgrad, _conv_dgrad) against a recording of the commit
before those three functions existed, when each autograd Function chose its kernels itself: the same launches, with the same
arguments, in the same order, pack launches and the stream included (tests/golden/conv_route_trace.json, written by
tests/golden/make_golden_conv_route.py; the scenarios and what a trace keeps: tests/conv_route_scenarios.py)."""
import json
import os

import pytest

import conv_route_scenarios as S

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route_trace.json")) as _f:
    GOLDEN = json.load(_f)
SCENARIOS = S.scenarios()


def test_the_recording_covers_every_scenario():
    assert sorted(GOLDEN["scenarios"]) == sorted(sc[0] for sc in SCENARIOS)


@pytest.mark.parametrize("sc", SCENARIOS, ids=[sc[0] for sc in SCENARIOS])
def test_launch_trace_equals_the_recording(sc):
    got, _ = S.run(sc)
    want = [GOLDEN["calls"][i] for i in GOLDEN["scenarios"][sc[0]]]
    got = json.loads(json.dumps(got))           # (tuples -> lists, as the file has them)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} of {len(want)}: {g} (recorded: {w}); before it: {got[max(0, i - 3):i]}"
    assert len(got) == len(want), f"{len(got)} launches, recorded {len(want)}; next: {(got + want)[min(len(got), len(want))]}"
