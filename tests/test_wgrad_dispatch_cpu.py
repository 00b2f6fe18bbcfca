"""CPU: which kernel the stride-1 weight gradient runs on (ops.wgrad_kernel_for, ops._wg4_plan_ok - thin lookups of the library's own
dispatch rule, pesr_conv3x3_wgrad_kernel / pesr_conv3x3_wgrad_wino4_side) against a recording of the Python re-typing of the planners
they replaced (tests/golden/wgrad_dispatch.json, written by tests/golden/make_golden_wgrad_dispatch.py at the commit before the query
existed).  One declared class of differences: the old mirror copied F(2,3)'s ragged-strip rule but not ww_plan's `tiles * split < 8`
rejection (csrc/conv3x3_wgrad_wino.hip), so it named the F(2,3) kernel for shapes the library has always run on the direct kernel.
Needs the built library (host-only entry points), no GPU."""
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_dispatch.json")
SWITCHES = ("USE_WGRAD_WINO", "USE_WGRAD_WINO4")
DIRECT, WINO23 = 0, 1        # indices into the recording's kernel list


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["points"] = [list(p) for p in itertools.product(*(g["grid"][k] for k in ("N", "H", "W", "Cin", "Cout")))] + g["extra"]
    return g


@pytest.fixture
def settings():
    """-> a function that puts ops into one recorded setting; everything it touches is put back (and the planner memo emptied) after."""
    from pesr_amd import ops
    saved = {k: getattr(ops, k) for k in SWITCHES + ("USE_WINO4",)}

    def apply(row):
        ops.USE_WINO4 = True
        for k in SWITCHES:
            setattr(ops, k, row["switches"][k])

    try:
        yield apply
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops._MEMO.clear()


def ww_plan_too_few_workgroups(N, H, W, Cin, Cout):
    """ww_plan's last rejection, restated (csrc/conv3x3_wgrad_wino.hip: 64 x 64 channel tiles, segments of one row x 24 x-tiles of two
    pixels, split-K over up to 256 / tiles slices rounded to whole strips): fewer than 8 workgroups."""
    tiles = (Cout // 64) * (Cin // 64)
    total = N * ((W // 2 + 23) // 24) * H
    split = max(1, min((256 + tiles - 1) // tiles, total))
    sps = (total + split - 1) // split
    if sps > H:
        sps = (sps + H - 1) // H * H
    return tiles * ((total + sps - 1) // sps) < 8


def test_recording_is_the_grid_the_issue_names(golden):
    assert golden["kernels"] == ["conv3x3_wgrad_kernel", "conv3x3_wgrad_wino_kernel", "conv3x3_wgrad_wino4_kernel",
                                 "conv3x3_wgrad_wino4x_kernel", "conv3x3_wgrad_wino4p_kernel"]
    assert golden["grid"] == {"N": [1, 2, 3, 5, 12, 13, 16], "H": [1, 2, 5, 24, 27, 48],
                              "W": [4, 8, 12, 16, 20, 24, 28, 44, 46, 48, 52, 92, 94, 96, 100, 142, 144],
                              "Cin": [32, 64, 128, 256], "Cout": [64, 96, 192, 512]}
    assert golden["extra"] == [[6, 22000, 8, 64, 512]]
    assert len(golden["points"]) == 7 * 6 * 17 * 4 * 4 + 1
    assert [r["name"] for r in golden["settings"]] == ["default", "USE_WGRAD_WINO=0", "USE_WGRAD_WINO4=0"]
    for r in golden["settings"]:
        assert len(r["kernel"]) == len(r["covered"]) == len(r["side"]) == len(golden["points"])
    default = golden["settings"][0]
    assert {s for s, c in zip(default["side"], default["covered"]) if c == "1"} == set("12346")      # every side the plan knows
    assert default["covered"][-1] == "0"                                                          # the 32-bit strip-offset rejection


def test_kernel_choice_reproduces_the_recording(golden, settings):
    from pesr_amd import ops
    names, fracs = golden["kernels"], golden["fracs"]
    exceptions, wino23_default = set(), 0
    for row in golden["settings"]:
        settings(row)
        for want, p in zip(row["kernel"], golden["points"]):
            want = int(want)
            name, frac = ops.wgrad_kernel_for(*p)
            if want == WINO23 and ww_plan_too_few_workgroups(*p):      # the declared class: the mirror lacked this rule of ww_plan
                assert (name, frac) == ("conv3x3_wgrad_kernel", 1.0), (row["name"], p, name, frac)
                exceptions.add(tuple(p))
                continue
            assert (name, frac) == (names[want], fracs[want]), (row["name"], p, name, frac)
            wino23_default += row["name"] == "default" and want == WINO23
    assert len(exceptions) >= 17, len(exceptions)
    assert {(1, 1, 48, 64, 64), (1, 2, 48, 64, 192), (1, 1, 144, 64, 64)} <= exceptions
    assert wino23_default >= 1          # F(2,3) is still chosen somewhere under the default setting (W = 94, 142)


def test_wino4_plan_reproduces_the_recording(golden, settings):
    """_wg4_plan_ok is the plan alone (no switch changes it): `covered` everywhere, `side` where covered."""
    from pesr_amd import ops
    for row in golden["settings"]:
        settings(row)
        for cov, side, p in zip(row["covered"], row["side"], golden["points"]):
            ok, s = ops._wg4_plan_ok(*p)
            assert ok == (cov == "1"), (row["name"], p)
            if ok:
                assert s == int(side), (row["name"], p, s)


def test_query_knows_the_rules_the_mirror_did_not():
    """ps_in (Cout % 256) and accumulate (no F(2,3) mode) take part in the library's rule; stride 2 and algo DIRECT are the direct kernel."""
    from pesr_amd import _lib
    q = _lib.lib().pesr_conv3x3_wgrad_kernel
    assert q(16, 48, 48, 256, 256, 1, 0, 0, 0) == 5 and q(16, 48, 48, 256, 256, 1, 1, 0, 0) == 5       # the G body, the upsampler conv
    assert q(16, 48, 48, 64, 192, 1, 1, 0, 0) == 0                       # ps_in, Cout % 256: neither Winograd form
    assert q(16, 48, 94, 64, 64, 1, 0, 0, 0) == 1 and q(16, 48, 94, 64, 64, 1, 0, 0, 1) == 0           # F(2,3) cannot accumulate
    assert q(16, 48, 48, 256, 256, 1, 0, 0, 1) == 5                      # ... the F(4,3) kernels can
    assert [q(16, 48, 48, 256, 256, 1, 0, a, 0) for a in (0, 1, 2, 5)] == [5, 0, 1, 4]
    assert q(16, 48, 48, 256, 256, 1, 0, 3, 0) < 0 and q(16, 48, 48, 256, 256, 1, 0, 4, 0) < 0        # the retired algorithms
    L = _lib.lib()           # ... which the call and the workspace query refuse too (a null workspace: nothing is launched either way)
    assert [L.pesr_conv3x3_wgrad(None, None, None, None, 16, 48, 48, 256, 256, 1, 1.0, 0, a, 0, None, 1 << 40, None) for a in (3, 4, 5)] == [-1, -1, -2]
    assert [L.pesr_conv3x3_wgrad_workspace_bytes(16, 48, 48, 256, 256, 1, a) > 0 for a in (3, 4, 5)] == [False, False, True]
    assert q(16, 24, 24, 256, 256, 1, 0, 5, 0) == 4                      # side by side strips: every F(4,3) kernel that is left does them
    assert q(16, 48, 48, 256, 256, 2, 0, 0, 0) == 0 and q(16, 48, 48, 256, 256, 1, 0, 6, 0) < 0
