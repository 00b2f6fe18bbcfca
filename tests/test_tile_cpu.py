"""CPU: tiled inference (docs/modes.md section 4h) without a GPU - the tile plan's properties and its equality with the
restatement's own arithmetic, receptive_halo against the float64 oracle, the restatement itself pinned with the exact toy model,
the flags of test.py / train.py, the host-side refusals of the two C-ABI entries, and the ISA of csrc/tile.hip (no fused
multiply-add)."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tile_oracle as TO
from helpers import x8_toy_model
from oracle import detrand
from scale_oracle import gen_sd_scaled, generator_forward_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- 1. the plan ------------------------------------------------------------------------------------------------------------------
def test_axis_plan_properties_and_restatement():
    from pesr_amd import tile
    for n in range(1, 71):
        for core in (1, 4, 8, 12, 16, 32):
            for halo in (0, 1, 3, 8):
                t, rows = tile.axis_plan(n, core, halo)
                assert (t, rows) == TO.axis(n, core, halo), (n, core, halo)
                assert t == min(core + 2 * halo, n) and len(rows) == -(-n // core)
                nxt = 0
                for start, lo, hi in rows:
                    assert 0 <= start and start + t <= n                      # same length, inside the axis
                    assert lo == nxt and lo < hi <= n                         # the owned intervals partition the axis
                    nxt = hi
                    assert start <= lo and hi <= start + t                    # owned inside the tile
                    assert start == 0 or lo - start >= halo                   # an owned pixel is >= halo from an edge that is no
                    assert start + t == n or start + t - hi >= halo           # image edge
                assert nxt == n


def test_plan_is_the_product_and_equals_the_restatement():
    from pesr_amd import tile
    sizes = [1, 2, 7, 13, 31, 37, 48, 53, 64, 67, 70]
    for H in sizes:
        for W in sizes:
            for core, halo in ((1, 0), (4, 1), (8, 3), (12, 8), (16, 0), (32, 8)):
                if core == 1 and H * W > 200:
                    continue
                th, tw, rows = tile.plan(H, W, core, halo)
                assert (th, tw, rows) == TO.tiles(H, W, core, halo)
                seen = np.zeros((H, W), dtype=np.int32)
                for y0, x0, oy, ox, oh, ow in rows:
                    assert 0 <= y0 and y0 + th <= H and 0 <= x0 and x0 + tw <= W
                    seen[oy:oy + oh, ox:ox + ow] += 1
                assert (seen == 1).all()
    with pytest.raises(ValueError):
        tile.axis_plan(10, 0, 1)
    with pytest.raises(ValueError):
        tile.axis_plan(10, 4, -1)
    assert tile.blend_weights(0.6) == (float(np.float32(0.6)), float(np.float32(1 - 0.6)))


# ---- 2. receptive_halo against the float64 oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("depth", [1, 2])
def test_receptive_halo_is_the_exact_one(depth, scale):
    from pesr_amd import tile
    halo = tile.receptive_halo(depth, scale)
    assert halo == 2 * depth + 4
    sd = {k: v.double() for k, v in gen_sd_scaled(16, depth, scale, seed=7).items()}
    img = detrand.image_batch((1, 3, 37, 53), 31).double()
    fn = lambda t: generator_forward_scaled(sd, t, depth, 0.1, scale)
    with torch.no_grad():
        whole = fn(img)
        at = float((TO.tiled(img, fn, scale, 8, halo) - whole).abs().max())
        below = float((TO.tiled(img, fn, scale, 8, halo - 1) - whole).abs().max())
    print(f"depth {depth} x{scale}: halo {halo}: {at:.3e}, halo {halo - 1}: {below:.3e}")
    assert at <= 1e-9
    assert below > 1e-6
    with pytest.raises(ValueError):
        tile.receptive_halo(2, 5)


# ---- 3. the restatement pinned with the exact toy model -------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,core,halo", [(37, 53, 8, 1), (37, 53, 8, 2), (13, 22, 16, 4), (48, 50, 12, 1), (9, 64, 8, 3)])
def test_restatement_equals_whole_image_bit_for_bit(H, W, core, halo):
    T = _load("test")
    model = x8_toy_model(11, 12)
    img = detrand.image_batch((1, 3, H, W), 500 + H + W)
    with torch.no_grad():
        assert torch.equal(TO.tiled(img, model, 2, core, halo), model(img))
        ens = lambda t: T.x8_forward(t, model)
        assert torch.equal(TO.tiled(img, ens, 2, core, halo), ens(img))


def test_a_lost_halo_cannot_pass():
    model = x8_toy_model(11, 12)
    img = detrand.image_batch((1, 3, 40, 40), 77)
    with torch.no_grad():
        d = float((TO.tiled(img, model, 2, 8, 0) - model(img)).abs().max())
    print("halo 0:", d)
    assert d > 1.0


# ---- 4. flags -------------------------------------------------------------------------------------------------------------------------
def test_flags_default_off_and_bad_values_exit():
    Te, Tr = _load("test"), _load("train")
    a = Te.build_parser().parse_args([])
    assert a.tile == 0 and a.tile_halo == -1 and a.tile_batch == 16
    a = Te.build_parser().parse_args(["--tile", "32", "--tile_halo", "8", "--tile_batch", "8"])
    assert (a.tile, a.tile_halo, a.tile_batch) == (32, 8, 8)
    for argv, flag in ((["--tile", "-1"], r"--tile\b"), (["--tile", "8", "--tile_halo", "-2"], "--tile_halo"),
                       (["--tile", "8", "--tile_batch", "0"], "--tile_batch")):
        with pytest.raises(SystemExit, match=flag):
            Te.main(argv)
    t = Tr.build_parser().parse_args([])
    assert t.valid_tile == 0 and t.valid_tile_halo == -1
    t = Tr.build_parser().parse_args(["--valid_tile", "16", "--valid_tile_halo", "4"])
    assert (t.valid_tile, t.valid_tile_halo) == (16, 4)
    Tr.check_limits(t, 1)
    for argv, flag in ((["--valid_tile", "-3"], r"--valid_tile\b"), (["--valid_tile", "8", "--valid_tile_halo", "-2"], "--valid_tile_halo")):
        with pytest.raises(SystemExit, match=flag):
            Tr.check_limits(Tr.build_parser().parse_args(argv), 1)
    from pesr_amd import tile
    assert "APPROXIMATION" in tile.describe(32, 8, 68) and "APPROXIMATION" not in tile.describe(32, 68, 68)


# ---- 5. refusals of the C ABI, on the host --------------------------------------------------------------------------------------------
def _d(rows):
    a = np.ascontiguousarray(np.array(rows, dtype=np.int32))
    return a, a.ctypes.data


def test_c_abi_refuses_before_anything_is_launched():
    """Both entries check their arguments and the HOST copy of the descriptor first: PESR_EINVAL comes back without a device (the
    device pointers are never followed on the host)."""
    from pesr_amd import _lib
    L = _lib.lib()
    p = 0x10000
    def g(rows, n=None, H=20, W=30, oh=8, ow=12, u8=0):
        arr, ptr = _d(rows)                                                   # (arr outlives the call)
        return L.pesr_tile_gather(p, u8, H, W, p, ptr, p, len(rows) if n is None else n, oh, ow, None)
    keep = [_d([(0, 0, 0)])]
    assert g([(13, 0, 0)]) == -1                                              # 13 + 8 > 20
    assert g([(0, 19, 0)]) == -1
    assert g([(-1, 0, 0)]) == -1
    assert g([(0, 0, 8)]) == -1                                               # member outside 0..7
    assert g([(9, 0, 4)]) == -1                                               # transposed: the tile is 12 x 8, 9 + 12 > 20
    assert g([(0, 0, 0)], n=0) == -1
    assert g([(0, 0, 0)], u8=2) == -1
    assert L.pesr_tile_gather(None, 0, 20, 30, p, keep[0][1], p, 1, 8, 12, None) == -1

    def s(rows, n, E, th=8, tw=8, sc=2, H=20, W=30, hi=None, outs=(p, None)):
        arr, ptr = _d(rows)
        return L.pesr_tile_scatter(p, hi, 0, None, 0, 1.0, 0.0, ptr, p, n, E, th, tw, sc, H, W, outs[0], outs[1], None)
    ok = (0, 0, 0, 0, 8, 8)
    assert s([ok], 1, 2) == -1                                                # E not 1 or 8
    assert s([ok], 12, 8) == -1                                               # E = 8 with a count that is no multiple of 8
    assert s([ok], 1, 1, sc=5) == -1 and s([ok], 1, 1, sc=1) == -1
    assert s([(13, 0, 13, 0, 4, 4)], 1, 1) == -1                              # tile outside the image
    assert s([(0, 0, 0, 0, 9, 8)], 1, 1) == -1                                # owned rectangle outside its tile
    assert s([(4, 4, 3, 4, 2, 2)], 1, 1) == -1
    assert s([(0, 0, 0, 0, 0, 8)], 1, 1) == -1                                # empty
    assert s([ok], 1, 1, outs=(None, None)) == -1                             # nowhere to write
    assert s([ok], 8, 8, th=8, tw=12) == -1                                   # one tensor holds eight members of square tiles only
    assert s([ok], 1, 1, hi=p) == -1


# ---- the ISA ---------------------------------------------------------------------------------------------------------------------------
def test_tile_kernels_hold_no_fused_multiply_add():
    from pesr_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + build.HIPCC_FLAGS + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "tile.hip"), "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    assert "tile_scatter_kernel" in asm and "tile_gather_kernel" in asm
    assert len(re.findall(r"\bv_(pk_)?(fma|fmac|mad|mac)_(f16|f32|f64|legacy|mix)", asm)) == 0
    assert len(re.findall(r"\bv_(pk_)?mul_f32\b", asm)) > 0 and len(re.findall(r"\bv_(pk_)?add_f32\b", asm)) > 0
