"""CPU: the definition of SSIM-Y with a border shave (docs/modes.md section 4g) - the float64 restatement tests/ssim_oracle.py against
closed forms and against an independent 2-D formulation (scipy), utils.compute_SSIM's host path against the restatement, the window
constants that ssim.hip carries, the absence of fused multiply-adds in the compiled kernel, refusals, the shave keyword of
utils.compute_PSNR and the new flags of test.py / train.py."""
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ssim_oracle as SO
from helpers import load_golden
from oracle import detrand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pair(seed, h, w, sigma=8.0):
    """A blocky uint8-valued image and a noisy copy of it, [3, h, w] float32."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (3, (h + 7) // 8, (w + 7) // 8)).astype(np.float64)
    a = np.kron(base, np.ones((8, 8)))[:, :h, :w]
    b = np.clip(np.rint(a + rng.normal(0.0, sigma, a.shape)), 0, 255)
    return a.astype(np.float32), b.astype(np.float32)


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------
def test_window_is_the_stated_gaussian():
    g = SO.window()
    assert len(g) == 11 and g == g[::-1] and abs(sum(g) - 1.0) < 1e-15
    assert abs(g[5] / g[4] - math.exp(1 / 4.5)) < 1e-15 and abs(g[5] / g[0] - math.exp(25 / 4.5)) < 1e-12      # sigma = 1.5
    assert abs(SO.C1 - 6.5025) < 1e-14 and abs(SO.C2 - 58.5225) < 1e-13


def test_image_against_itself_is_exactly_one():
    a, _ = _pair(1, 37, 53)
    m = SO.ssim_map(a, a)
    assert m.shape == (27, 43) and np.all(m == 1.0)
    assert SO.ssim(a, a) == 1.0


@pytest.mark.parametrize("c,d", [(0, 255), (16, 235), (100, 101), (200, 30), (7, 7)])
def test_constant_images_closed_form(c, d):
    # luma of a grey pixel (v, v, v) is computed by the definition itself: the closed form is stated on Y
    x = np.full((15, 18), float(c))
    y = np.full((15, 18), float(d))
    m = SO.ssim_map_y(x, y)
    want = (2.0 * c * d + SO.C1) / (c * c + d * d + SO.C1)
    assert m.shape == (5, 8)
    assert np.max(np.abs(m - want)) <= 1e-12


def test_swapping_the_images_gives_the_same_bits():
    a, b = _pair(2, 40, 29)
    assert np.array_equal(SO.ssim_map(a, b), SO.ssim_map(b, a))
    assert np.array_equal(SO.ssim_map(a, b, 3), SO.ssim_map(b, a, 3))


@pytest.mark.parametrize("shave", [1, 2, 4])
def test_shave_equals_the_sliced_arrays(shave):
    a, b = _pair(3, 33, 47)
    assert np.array_equal(SO.ssim_map(a, b, shave), SO.ssim_map(a[:, shave:-shave, shave:-shave], b[:, shave:-shave, shave:-shave]))
    assert SO.ssim_map(a, b, shave).shape == (33 - 2 * shave - 10, 47 - 2 * shave - 10)


def test_luma_is_the_rounded_y_of_the_psnr():
    U = _load("utils")
    rng = np.random.default_rng(4)
    t = rng.uniform(-20, 280, (3, 19, 23)).astype(np.float32)
    [img] = U.tensors_to_imgs([torch.from_numpy(t)[None]])
    want = np.clip(U.rgb2y(img.astype(np.float64)), 0, 255).round()
    assert np.array_equal(SO.luma(t), want)
    assert SO.luma(t).min() >= 16 and SO.luma(t).max() <= 235


# ---- 2. an independent formulation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,h,w", [(10, 48, 48), (11, 31, 57), (12, 11, 11)])
def test_restatement_against_direct_2d_correlation(seed, h, w):
    sig = pytest.importorskip("scipy.signal")
    a, b = _pair(seed, h, w)
    x, y = SO.luma(a), SO.luma(b)
    g = np.array(SO.window())
    win = np.outer(g, g)

    def f(v):
        return sig.correlate2d(v, win, mode="valid")

    mx, my = f(x), f(y)
    sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    want = ((2 * mx * my + SO.C1) * (2 * sxy + SO.C2)) / ((mx * mx + my * my + SO.C1) * (sx + sy + SO.C2))
    got = SO.ssim_map(a, b)
    assert got.shape == want.shape == (h - 10, w - 10)
    diff = float(np.max(np.abs(got - want)))
    print(f"{h} x {w}: restatement vs correlate2d, max |diff| = {diff:.3e}")
    assert diff <= 1e-12


# ---- 3. utils.compute_SSIM, host path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,h,w,shave", [(20, 97, 131, 0), (21, 11, 11, 0), (22, 40, 64, 4), (23, 30, 21, 2)])
def test_compute_ssim_host_path_against_the_restatement(seed, h, w, shave):
    U = _load("utils")
    a, b = _pair(seed, h, w)
    if seed == 22:                                     # a generator-like output: non-integer and out-of-range values
        b = (b.astype(np.float64) * 1.2 - 20.3).astype(np.float32)
    m = SO.ssim_map(a, b, shave)
    want = math.fsum(m.ravel().tolist()) / m.size
    got = U.compute_SSIM(torch.from_numpy(a)[None], torch.from_numpy(b)[None], shave)
    assert isinstance(got, float)
    diff = abs(got - want)
    print(f"{h} x {w} shave {shave}: host path {got!r}, restatement {want!r}, |diff| = {diff:.3e}")
    assert diff <= (m.size - 1) * 2.0 ** -53 + 1e-12
    assert U.compute_SSIM(a, b, shave) == got          # arrays and [3, H, W] are taken too


def test_host_window_and_kernel_literals_are_the_restatements():
    from pesr_amd import ops
    assert list(ops.SSIM_WINDOW) == SO.window()
    src = open(os.path.join(ROOT, "pesr_amd", "csrc", "ssim.hip")).read()
    body = src[src.index("constexpr double ssim_g"):]
    body = body[:body.index("}")]
    lits = [float(v) for v in re.findall(r"[:?]\s*(0\.\d+)", body)]
    assert lits == SO.window()[5::-1]                  # d = 0 .. 5 from the centre outwards


def test_kernel_has_no_fused_multiply_add_outside_the_division():
    """Every v_fma_f64 / v_fmac_f64 of ssim.hip's device code belongs to the expansion of an IEEE double division (3 + 2 per
    division, next to one v_div_fmas_f64 and one v_div_fixup_f64): none is left for the filter and the map arithmetic."""
    from pesr_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + build.HIPCC_FLAGS + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "ssim.hip"), "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    count = lambda pat: len(re.findall(pat, asm))
    divs = count(r"\bv_div_fixup_f64\b")
    assert divs >= 2 and count(r"\bv_div_fmas_f64\b") == divs
    assert count(r"\bv_fma_f64\b") == 3 * divs and count(r"\bv_fmac_f64") == 2 * divs
    assert count(r"\bv_pk_fma") == 0 and count(r"\bv_mul_f64\b") > 100 and count(r"\bv_add_f64\b") > 100


# ---- 4. refusals, flags, the shave keyword of compute_PSNR ------------------------------------------------------------------------
def test_refusals():
    U = _load("utils")
    a, b = _pair(30, 14, 20)
    with pytest.raises(ValueError):
        SO.ssim_map(a, b, 2)                           # 10 x 16 after the shave
    with pytest.raises(ValueError):
        SO.ssim_map(a[:, :10], b[:, :10])
    with pytest.raises(ValueError):
        SO.ssim_map(a, b[:, :, :19])
    with pytest.raises(ValueError):
        SO.ssim_map(a, b, -1)
    ta, tb = torch.from_numpy(a)[None], torch.from_numpy(b)[None]
    assert isinstance(U.compute_SSIM(ta, tb, 1), float)                  # 12 x 18: still a window
    with pytest.raises(ValueError):
        U.compute_SSIM(ta, tb, 2)
    with pytest.raises(ValueError):
        U.compute_SSIM(ta[..., :10], tb[..., :10])
    with pytest.raises(ValueError):
        U.compute_SSIM(ta, tb[..., :19])
    with pytest.raises(ValueError):
        U.compute_SSIM(ta, tb, -1)


def test_flags_default_off_and_ssim_needs_from_hr(capsys):
    Te, Tr = _load("test"), _load("train")
    a = Te.build_parser().parse_args([])
    assert a.ssim is False and a.shave == 0
    b = Te.build_parser().parse_args(["--ssim", "true", "--shave", "-1"])
    assert b.ssim is True and b.shave == -1
    t = Tr.build_parser().parse_args([])
    assert t.valid_ssim is False and t.valid_shave == 0
    t = Tr.build_parser().parse_args(["--valid_ssim", "true", "--valid_shave", "4"])
    assert t.valid_ssim is True and t.valid_shave == 4
    with pytest.raises(SystemExit, match="--from_hr true"):
        Te.main(["--ssim", "true"])
    with pytest.raises(SystemExit, match="--from_hr true"):
        Te.main(["--ssim", "true", "--from_hr", "false", "--dataset", "nowhere"])


def test_compute_psnr_shave_keyword():
    U = _load("utils")
    g = load_golden("gv9_utils")
    a = detrand.image_batch((1, 3, 16, 20), 41)
    b = a + detrand.uniform((1, 3, 16, 20), 42, -20, 20)
    plain = U.compute_PSNR(a.clone(), b.clone())
    assert plain == U.compute_PSNR(a.clone(), b.clone(), shave=0) == U.compute_PSNR(a.clone(), b.clone(), 0)
    assert abs(plain - float(g["psnr"])) < 1e-9
    want = U.compute_PSNR(a[:, :, 2:-2, 2:-2].clone(), b[:, :, 2:-2, 2:-2].clone())
    assert U.compute_PSNR(a.clone(), b.clone(), shave=2) == want and want != plain
    ya, yb = SO.luma(a[0].numpy())[2:-2, 2:-2], SO.luma(b[0].numpy())[2:-2, 2:-2]
    assert abs(want - 20 * math.log10(255 / math.sqrt(float(np.mean((ya - yb) ** 2))))) < 1e-9
    with pytest.raises(ValueError):
        U.compute_PSNR(a, b, shave=8)


def test_c_abi_refuses_before_anything_is_launched():
    """pesr_ssim_y checks its arguments on the host first: PESR_EINVAL / PESR_EWORKSPACE come back without a device (the pointers
    are never followed on the host)."""
    from pesr_amd import _lib
    lib = _lib.lib()
    p = 0x10000
    assert lib.pesr_ssim_y(p, p, p, 1, 10, 64, 0, 0, 0, None, p, 1 << 20, None) == -1          # height below the window
    assert lib.pesr_ssim_y(p, p, p, 1, 64, 18, 0, 0, 4, None, p, 1 << 20, None) == -1          # 18 - 8 = 10 columns left
    assert lib.pesr_ssim_y(p, p, p, 1, 64, 64, 0, 0, -1, None, p, 1 << 20, None) == -1
    assert lib.pesr_ssim_y(p, p, p, 0, 64, 64, 0, 0, 0, None, p, 1 << 20, None) == -1
    assert lib.pesr_ssim_y(None, p, p, 1, 64, 64, 0, 0, 0, None, p, 1 << 20, None) == -1
    assert lib.pesr_ssim_y(p, p, p, 1, 2040, 1356, 0, 0, 0, None, p, 64, None) == -2           # far more than 8 workgroups
    assert lib.pesr_ssim_y(p, p, p, 1, 64, 64, 0, 0, 0, None, None, 0, None) == -2
