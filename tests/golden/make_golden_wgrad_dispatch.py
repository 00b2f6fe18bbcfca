"""Writes wgrad_dispatch.json: which kernel ops.wgrad_kernel_for names for the stride-1 weight gradient, and what ops._wg4_plan_ok
says of the F(4,3) plan, over a grid of problems and under the settings of the USE_WGRAD_* switches - as answered by the commit this
script is run at.  It was run at the commit BEFORE the library's own query (pesr_conv3x3_wgrad_kernel) existed, when both functions
re-typed the planners of csrc/conv3x3_wgrad_wino4.hip / conv3x3_wgrad_wino.hip in Python; tests/test_wgrad_dispatch_cpu.py holds the
library's answer to that recording.  (It then had two more switches and settings, for two F(4,3) kernels retired since: their rows
were filtered out of the recording, the rest of it is as written then - which is why kernel names 2 and 3 are still in its list.)  No GPU.  Run from the repository root: python tests/golden/make_golden_wgrad_dispatch.py
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pesr_amd import ops  # noqa: E402

KERNELS = ["conv3x3_wgrad_kernel", "conv3x3_wgrad_wino_kernel", "conv3x3_wgrad_wino4_kernel", "conv3x3_wgrad_wino4x_kernel",
           "conv3x3_wgrad_wino4p_kernel"]          # the file stores indices into this list
FRACS = [1.0, 2.0 / 3.0, 0.5, 0.5, 1.0 / 3.0]       # ... and the fraction is a function of the kernel under these settings
GRID = {"N": [1, 2, 3, 5, 12, 13, 16],
        "H": [1, 2, 5, 24, 27, 48],
        "W": [4, 8, 12, 16, 20, 24, 28, 44, 46, 48, 52, 92, 94, 96, 100, 142, 144],
        "Cin": [32, 64, 128, 256],
        "Cout": [64, 96, 192, 512]}
EXTRA = [[6, 22000, 8, 64, 512]]                    # the 32-bit strip-offset rejection of the side-by-side form (planner only)
SWITCHES = ("USE_WGRAD_WINO", "USE_WGRAD_WINO4")
SETTINGS = [("default", {}), ("USE_WGRAD_WINO=0", {"USE_WGRAD_WINO": False}), ("USE_WGRAD_WINO4=0", {"USE_WGRAD_WINO4": False})]
DEFAULTS = {"USE_WGRAD_WINO": True, "USE_WGRAD_WINO4": True}


def points():
    """The grid in file order: itertools.product over GRID's keys as listed, the last one fastest; then EXTRA."""
    return [list(p) for p in itertools.product(*(GRID[k] for k in ("N", "H", "W", "Cin", "Cout")))] + EXTRA


def main():
    saved = {k: getattr(ops, k) for k in SWITCHES}
    saved_wino4 = ops.USE_WINO4
    ops.USE_WINO4 = True
    rows = []
    try:
        for name, over in SETTINGS:
            sw = dict(DEFAULTS, **over)
            for k, v in sw.items():
                setattr(ops, k, v)
            kern, covered, side = [], [], []
            for p in points():
                kname, frac = ops.wgrad_kernel_for(*p)
                assert frac == FRACS[KERNELS.index(kname)], (name, p, kname, frac)
                ok, s = ops._wg4_plan_ok(*p)
                kern.append(str(KERNELS.index(kname)))
                covered.append("1" if ok else "0")
                side.append(str(s) if ok else "0")
            rows.append({"name": name, "switches": sw, "kernel": "".join(kern), "covered": "".join(covered), "side": "".join(side)})
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.USE_WINO4 = saved_wino4
    with open(os.path.join(HERE, "wgrad_dispatch.json"), "w") as f:
        json.dump({"kernels": KERNELS, "fracs": FRACS, "grid": GRID, "extra": EXTRA, "settings": rows}, f, separators=(",", ":"))
        f.write("\n")
    print({r["name"]: ([r["kernel"].count(str(i)) for i in range(5)], {s: r["side"].count(s) for s in "012346"}) for r in rows})


if __name__ == "__main__":
    main()
