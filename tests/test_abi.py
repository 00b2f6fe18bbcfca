"""CPU: the C-ABI shared library builds, loads without a GPU and exports every symbol include/pesr_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pesr_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from pesr_amd import build
    lib_path = build.build(force=False, verbose=False)     # hipcc cross-compiles for gfx950 without a GPU
    lib = ctypes.CDLL(lib_path)
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/pesr_hip.h but not exported by libpesr_hip.so"
    assert lib.pesr_abi_version() == 20


def test_ctypes_signatures_cover_the_header():
    from pesr_amd import _lib
    assert sorted(_lib.SIGNATURES) == header_symbols()
    _lib.lib()   # binds argtypes/restype for every entry; raises if anything is missing


def test_no_cpu_fallback():
    import torch
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.conv3x3_fwd(torch.zeros(1, 4, 4, 16), torch.zeros(9 * 16 * 64), None, 64)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under pesr_amd/, model/, train.py, test.py may import it."""
    bad = []
    for base in ("pesr_amd", "model"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith(".py"):
                    txt = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M):
                        bad.append(os.path.join(dp, f))
    for f in ("train.py", "test.py"):
        p = os.path.join(ROOT, f)
        if os.path.exists(p) and re.search(r"^\s*(from|import)\s+oracle\b", open(p).read(), flags=re.M):
            bad.append(p)
    assert not bad, bad


def test_wino4_planner_scores_on_the_host():
    """pesr_conv3x3_wino4_score is host-only code (the F(4,3) kernel's tile planner): per-mille of the tiles' x-tile slots that
    hold real pixels, 0 when the shape is unsupported or yields fewer than 192 workgroups.  It decides the dispatch, so its
    behaviour on the shapes of the three networks is pinned here, without a GPU."""
    from pesr_amd import _lib
    score = _lib.lib().pesr_conv3x3_wino4_score
    assert score(16, 48, 48, 256, 256, 1) == 1000                 # G body: 12 rows x 12 x-tiles per tile, one round of 256 workgroups
    assert score(16, 96, 96, 256, 1024, 0) == 1000                # upsampler conv (fused PixelShuffle: no split-K)
    assert score(16, 24, 24, 512, 512, 1) == 1000                 # VGG conv4_x: 6-x-tile rows (dense LDS layout), split-K
    s12 = score(16, 12, 12, 512, 512, 1)                          # VGG conv5_x: 16 images stacked into one 207-row image
    assert 780 <= s12 <= 800, s12
    assert score(2, 12, 12, 512, 512, 1) == 0                     # too few workgroups even stacked and split
    assert score(1, 48, 48, 256, 256, 1) == 0                     # one image: 16 workgroups
    assert score(16, 48, 50, 256, 256, 1) == 0                    # width not a multiple of 4
    assert score(16, 48, 48, 256, 96, 1) == 0                     # Cout not a multiple of 64
