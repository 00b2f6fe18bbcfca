"""CPU: the table-driven choice of the 3x3 conv kernel family (ops._FAMILIES, ops.conv3x3_family_fwd / _dgrad, and through them
functional.PackedConvWeights.for_fwd / for_dgrad) against a recording of the `if` chains it replaced
(tests/golden/conv_dispatch.json, written by tests/golden/make_golden_dispatch.py at the commit before the table).  Needs the built
library for the planners' host-only score entry points, no GPU."""
import itertools
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["points"] = list(itertools.product(*(g["grid"][k] for k in ("N", "HW", "Cin", "Cout", "stride", "ps"))))
    return g


@pytest.fixture
def settings(golden):
    """-> a function that puts ops into one recorded setting; everything it touches is put back (and the planner memo emptied) after."""
    from pesr_amd import ops
    saved = ops.PRECISION, ops.USE_WINO, ops.USE_WINO4, ops.BF16_MIN_WGS

    def apply(row):
        ops.set_precision(row["precision"])
        ops.USE_WINO, ops.USE_WINO4, ops.BF16_MIN_WGS = row["USE_WINO"], row["USE_WINO4"], golden["BF16_MIN_WGS"]

    try:
        yield apply
    finally:
        ops.PRECISION, ops.USE_WINO, ops.USE_WINO4, ops.BF16_MIN_WGS = saved
        ops._MEMO.clear()


def test_recording_covers_every_family(golden):
    """Every family is the answer somewhere in the forward rows and somewhere in the dgrad rows; the two bf16 families under their own
    precision only; the grid is the one the recording says it is."""
    fams = golden["families"]
    assert fams == ["split-bf16", "bf16", "F(4,3)", "F(2,3)", "direct"]
    assert len(golden["points"]) == 3 * 7 * 5 * 5 * 2 * 2 and len(golden["settings"]) == 5
    for which in ("fwd", "dgrad"):
        for i, fam in enumerate(fams):
            where = {r["precision"] for r in golden["settings"] if str(i) in r[which]}
            assert where, (fam, which)
            if fam in ("bf16", "split-bf16"):
                assert where == {fam}, (fam, which, where)
        assert all(len(r[which]) == len(golden["points"]) for r in golden["settings"])


def test_family_selection_reproduces_the_recording(golden, settings):
    from pesr_amd import ops
    fams = golden["families"]
    assert [f.name for f in ops._FAMILIES] == fams            # the tuple's order IS the dispatch priority
    for row in golden["settings"]:
        settings(row)
        for which, pick in (("fwd", ops.conv3x3_family_fwd), ("dgrad", ops.conv3x3_family_dgrad)):
            for want, (N, (H, W), Cin, Cout, stride, ps) in zip(row[which], golden["points"]):
                got = pick(N, H, W, Cin, Cout, stride, ps)
                assert got.name == fams[int(want)], (row["precision"], row["USE_WINO"], row["USE_WINO4"], which, N, H, W, Cin, Cout, stride, ps)


def test_packed_conv_weights_build_the_recorded_familys_slot(golden, settings, monkeypatch):
    """for_fwd / for_dgrad ask for exactly that family's packing (mode 0 / 1) and keep it in the slot of its batched-re-pack mode number;
    the pack itself is replaced by a marker, so no GPU is needed.  Every 7th grid point of every setting: 1500 points."""
    from pesr_amd import functional as PF
    from pesr_amd import ops
    monkeypatch.setattr(ops, "_pack", lambda f, w, mode, ps: (f.name, mode, bool(ps)))
    fams = golden["families"]
    base = {f.name: f.mode for f in ops._FAMILIES}
    assert base == {"direct": 0, "F(2,3)": 2, "F(4,3)": 4, "bf16": 7, "split-bf16": 9}
    weights, n = {}, 0
    for row in golden["settings"]:
        settings(row)
        for j in range(0, len(golden["points"]), 7):
            N, (H, W), Cin, Cout, stride, ps = golden["points"][j]
            w = weights.get((Cout, Cin))
            if w is None:
                w = weights[(Cout, Cin)] = torch.empty(Cout, Cin, 3, 3)
            cache = PF.PackedConvWeights(ps=ps)
            f, d = fams[int(row["fwd"][j])], fams[int(row["dgrad"][j])]
            assert cache.for_fwd(w, (N, H, W, Cin), stride) == (f, 0, ps), (row["precision"], golden["points"][j])
            assert cache.for_dgrad(w, (N, H, W, Cin), stride) == (d, 1, ps), (row["precision"], golden["points"][j])
            (slot,) = cache._slots.values()
            assert set(slot.packs) == {base[f], base[d] + 1}
            n += 1
    assert n >= 200
