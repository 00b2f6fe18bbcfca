"""Writes conv_dispatch.json: which 3x3 conv kernel family PackedConvWeights.for_fwd / for_dgrad choose over a grid of problems,
as decided by the commit this script is run at.  The two `if` chains below restate pesr_amd/functional.py's for_fwd / for_dgrad of
the commit BEFORE the family table existed, in terms of the public ops.*_eligible functions only - so the file is a recording of
that commit's dispatch, and tests/test_conv_families_cpu.py holds the table-driven selection to it.  Needs the built library (the
host-only score entry points), no GPU.  Run from the repository root: python tests/golden/make_golden_dispatch.py
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pesr_amd import ops  # noqa: E402

FAMILIES = ["split-bf16", "bf16", "F(4,3)", "F(2,3)", "direct"]      # dispatch priority; the file stores indices into this list
GRID = {"N": [1, 4, 16],
        "HW": [[12, 12], [24, 24], [48, 48], [96, 96], [7, 48], [48, 50], [30, 36]],
        "Cin": [3, 32, 64, 256, 512],
        "Cout": [3, 64, 128, 256, 1024],
        "stride": [1, 2],
        "ps": [False, True]}
# (precision, USE_WINO, USE_WINO4)
SETTINGS = [("fp32", True, True), ("bf16", True, True), ("split-bf16", True, True), ("fp32", True, False), ("fp32", False, True)]
BF16_MIN_WGS = 64


def points():
    """The grid in file order: itertools.product over GRID's keys as listed, the last one fastest."""
    return itertools.product(*(GRID[k] for k in ("N", "HW", "Cin", "Cout", "stride", "ps")))


def family_fwd(N, H, W, Cin, Cout, stride, ps):
    if ops.bf16x3_eligible(N, H, W, Cin, Cout, stride, ps_out=ps):
        return "split-bf16"
    if ops.bf16_eligible(N, H, W, Cin, Cout, stride, ps_out=ps):
        return "bf16"
    if ops.wino4_eligible(N, H, W, Cin, Cout, stride, ps_out=ps):
        return "F(4,3)"
    if ops.wino_eligible(N, H, W, Cin, Cout, stride):
        return "F(2,3)"
    return "direct"


def family_dgrad(N, H, W, Cin, Cout, stride, ps):
    if stride == 1 and ops.bf16x3_eligible(N, H, W, Cout, Cin, 1, ps_in=ps):
        return "split-bf16"
    if stride == 1 and ops.bf16_eligible(N, H, W, Cout, Cin, 1, ps_in=ps):
        return "bf16"
    if stride == 2 and not ps and ops.bf16_s2_dgrad_eligible(N, H, W, Cout, Cin):
        return "bf16"
    if ops.wino4_eligible(N, H, W, Cout, Cin, stride):
        return "F(4,3)"
    if ops.wino_eligible(N, H, W, Cout, Cin, stride):
        return "F(2,3)"
    return "direct"


def main():
    saved = ops.PRECISION, ops.USE_WINO, ops.USE_WINO4, ops.BF16_MIN_WGS
    ops.BF16_MIN_WGS = BF16_MIN_WGS
    settings = []
    try:
        for precision, wino, wino4 in SETTINGS:
            ops.set_precision(precision)
            ops.USE_WINO, ops.USE_WINO4 = wino, wino4
            row = {"precision": precision, "USE_WINO": wino, "USE_WINO4": wino4}
            for name, pick in (("fwd", family_fwd), ("dgrad", family_dgrad)):
                row[name] = "".join(str(FAMILIES.index(pick(N, H, W, Cin, Cout, stride, ps))) for N, (H, W), Cin, Cout, stride, ps in points())
            settings.append(row)
    finally:
        ops.PRECISION, ops.USE_WINO, ops.USE_WINO4, ops.BF16_MIN_WGS = saved
    for name in ("fwd", "dgrad"):       # every family is the answer somewhere, the bf16 ones under their own precision only
        for i, fam in enumerate(FAMILIES):
            where = {r["precision"] for r in settings if str(i) in r[name]}
            assert where, f"{fam} is never chosen in the {name} rows: widen the grid"
            assert fam not in ("bf16", "split-bf16") or where == {fam}, (fam, name, where)
    with open(os.path.join(HERE, "conv_dispatch.json"), "w") as f:
        json.dump({"families": FAMILIES, "grid": GRID, "BF16_MIN_WGS": BF16_MIN_WGS, "settings": settings}, f, separators=(",", ":"))
        f.write("\n")
    print({(r["precision"], r["USE_WINO"], r["USE_WINO4"], n): [r[n].count(str(i)) for i in range(5)] for r in settings for n in ("fwd", "dgrad")})


if __name__ == "__main__":
    main()
