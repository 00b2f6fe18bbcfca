"""CPU: SSIM-Y as a training loss (docs/modes.md section 4p) - the ordered restatement of the gradient (tests/ssim_loss_oracle.py)
against torch.autograd on the float64 definition, the closed forms of the score, the constants and the absence of fused multiply-adds
in ssim.hip (the loss's kernels beside the score's), the refusals of the two C entry points, of train.py --alpha_ssim and of the
Trainer."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ssim_loss_cases as C
import ssim_loss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_ssim_loss_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- 1. the ordered gradient is the derivative of the definition ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(11, 11), (11, 58), (13, 29), (27, 59), (43, 107)])
def test_grad_ordered_against_autograd_on_the_float64_definition(h, w, n):
    """Before the rounding to float32: 1e-11 of the image's largest gradient (an unordered float64 evaluation of the formula was measured
    at 8.2e-15; the margin covers the kernel's own order).  After it: one float32 rounding, 2^-24 |value|, more."""
    a, b, g = C.case("noise", n, h, w)
    assert a.min() < 0 and a.max() > 255                              # nothing is clipped: such values take part
    exact = O.grad_exact(a, b, g)
    raw = O.grad_ordered(a, b, g, rounded=False)
    got = O.grad_ordered(a, b, g)
    assert got.dtype == np.float32 and raw.dtype == np.float64 and got.shape == raw.shape == exact.shape == (n, 3, h, w)
    for i in range(n):
        gmax = float(np.abs(exact[i]).max())
        e_raw = float(np.abs(raw[i] - exact[i]).max()) / gmax
        over = np.abs(got[i].astype(np.float64) - exact[i]) - (1e-11 * gmax + 2.0 ** -24 * np.abs(exact[i]))
        print(f"{n} x {h} x {w} image {i}: max |grad_ordered - autograd| = {e_raw:.3e} of max |grad| {gmax:.3e} before the rounding; "
              f"after it the worst excess over the allowance is {float(over.max()):.3e}")
        assert gmax > 0 and e_raw <= 1e-11
        assert float(over.max()) <= 0.0


def test_images_do_not_mix_and_g_is_linear():
    a, b, g = C.case("noise", 3, 13, 15)
    assert len(set(g.tolist())) == 3
    base = O.grad_ordered(a, b, g)
    for i in range(3):
        assert np.array_equal(O.grad_ordered(a[i:i + 1], b[i:i + 1], g[i:i + 1])[0], base[i])
    zero = O.grad_ordered(a, b, np.array([g[0], 0.0, g[2]]))
    assert bool((zero[1] == 0).all()) and np.array_equal(zero[0], base[0])


# ---- 2. the score --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(11, 11), (27, 59), (47, 80)])
def test_equal_images_score_exactly_one(h, w):
    """With equal inputs numerator and denominator are the same operations on the same bits: every window is 1.0, and so is the mean."""
    a, b, _ = C.case("same", 3, h, w)
    assert np.array_equal(a, b) and a.min() < 0 and a.max() > 255
    assert bool((O.map_ordered(a, b) == 1.0).all())
    assert O.score_ordered(a, b).tolist() == [1.0, 1.0, 1.0]


def test_constant_images_closed_form_and_unrounded_luma():
    a, b, _ = C.case("const", 1, 16, 33)
    x, y = float(O.luma(a[0])[0, 0]), float(O.luma(b[0])[0, 0])
    assert x != round(x) and abs(y - x - 3.0 * sum(O.KY)) < 1e-12      # the luma keeps its fraction
    want = (2.0 * x * y + O.C1) / (x * x + y * y + O.C1)
    assert np.max(np.abs(O.map_ordered(a, b) - want)) <= 1e-12 and abs(O.score_ordered(a, b)[0] - want) <= 1e-12


def test_score_ordered_is_the_mean_of_the_map():
    """The device's summation tree against an exact sum: (count - 1) roundings at most."""
    import math
    for h, w in ((13, 15), (47, 80), (60, 300)):                       # the last: 30 tiles ... and (below) more partials than lanes
        a, b, _ = C.case("noise", 1, h, w)
        m = O.map_ordered(a, b)[0]
        want = math.fsum(m.ravel().tolist()) / m.size
        assert abs(O.score_ordered(a, b)[0] - want) <= m.size * 2.0 ** -53
    m = np.random.default_rng(5).uniform(0.0, 1.0, (16 * 20, 32 * 15))  # 300 tiles: the final pass's second round
    assert abs(O._mean_ordered(m) - math.fsum(m.ravel().tolist()) / m.size) <= m.size * 2.0 ** -53


# ---- 3. what the kernel file carries ------------------------------------------------------------------------------------------------------
def test_kernel_literals_are_the_restatements():
    from pesr_amd import ops
    assert list(ops.SSIM_WINDOW) == O.window()
    src = open(os.path.join(ROOT, "pesr_amd", "csrc", "ssim.hip")).read()
    body = src[src.index("constexpr double ssim_g"):]
    body = body[:body.index("}")]
    assert [float(v) for v in re.findall(r"[:?]\s*(0\.\d+)", body)] == O.window()[5::-1]      # d = 0 .. 5 from the centre outwards
    assert "65.738 / 256" in src and "129.057 / 256" in src and "25.064 / 256" in src
    tile = re.search(r"SsimLossTile = SsimTile<(\d+), (\d+),", src)
    assert (int(tile.group(1)), int(tile.group(2))) == (O.TILE_H, O.TILE_W)                   # the score's summation order


def test_kernels_have_no_fused_multiply_add_outside_the_divisions():
    """As tests/test_ssim_cpu.py, for the file with all three kernels in it (one division in the score, six in the loss's forward, one
    in its backward): every v_fma_f64 / v_fmac_f64 belongs to the expansion of an IEEE double division."""
    from pesr_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + build.HIPCC_FLAGS + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "ssim.hip"), "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    count = lambda pat: len(re.findall(pat, asm))
    divs = count(r"\bv_div_fixup_f64\b")
    assert divs >= 8 and count(r"\bv_div_fmas_f64\b") == divs
    assert count(r"\bv_fma_f64\b") == 3 * divs and count(r"\bv_fmac_f64") == 2 * divs
    assert count(r"\bv_pk_fma") == 0 and count(r"\bv_mul_f64\b") > 100 and count(r"\bv_add_f64\b") > 100


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_anything_is_launched():
    """Both entry points check their arguments on the host first: PESR_EINVAL / PESR_EWORKSPACE come back without a device (the
    pointers are never followed on the host)."""
    from pesr_amd import _lib
    assert "pesr_ssim_loss_fwd" in _lib.SIGNATURES and "pesr_ssim_loss_bwd" in _lib.SIGNATURES
    lib = _lib.lib()
    p, big = 0x10000, 1 << 20
    fwd = lambda N, H, W, a=p, b=p, s=p, coef=None, ws=p, nb=big: lib.pesr_ssim_loss_fwd(a, b, s, N, H, W, 0, 1, coef, ws, nb, None)
    bwd = lambda N, H, W, a=p, b=p, coef=p, g=p, ga=p: lib.pesr_ssim_loss_bwd(a, b, coef, g, ga, N, H, W, 1, 0, None)
    for call in (fwd, bwd):
        assert call(1, 10, 64) == -1 and call(1, 64, 10) == -1 and call(1, 0, 0) == -1          # a side below the window
        assert call(0, 64, 64) == -1 and call(-1, 64, 64) == -1 and call(65536, 64, 64) == -1
        assert call(1, 64, 64, a=None) == -1 and call(1, 64, 64, b=None) == -1
    assert fwd(1, 64, 64, s=None) == -1 and fwd(1, 64, 64, s=p + 4) == -1 and fwd(1, 64, 64, coef=p + 4) == -1
    assert fwd(16, 192, 192, nb=8 * 16 * 12 * 6 - 1) == -2 and fwd(1, 64, 64, ws=None, nb=0) == -2
    assert fwd(1, 11, 11, coef=p, nb=7) == -2                          # a single window still needs its one partial
    assert bwd(1, 64, 64, coef=None) == -1 and bwd(1, 64, 64, g=None) == -1 and bwd(1, 64, 64, ga=None) == -1
    assert bwd(1, 64, 64, coef=p + 4) == -1 and bwd(1, 64, 64, g=p + 4) == -1 and bwd(1, 64, 64, ga=p + 2) == -1
    assert lib.pesr_abi_version() == 20


def test_ops_refuse_host_tensors():
    from pesr_amd import _lib, ops
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.ssim_loss_fwd(x, x)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.ssim_loss_bwd(x, x, torch.zeros(1, 3, 6, 6, dtype=torch.float64), torch.ones(1, dtype=torch.float64))


def test_train_flag_default_off_and_refusals(monkeypatch):
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise AssertionError("torch.cuda was initialised")
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    Tr = _load("train")
    d = Tr.build_parser().parse_args([])
    assert d.alpha_ssim == 0.0
    Tr.loss_terms_of(d)
    Tr.loss_terms_of(Tr.build_parser().parse_args(["--patch_size", "2"]))                   # off: any size
    for phase in ("pretrain", "train"):
        with pytest.raises(SystemExit, match=r"train\.py: --alpha_ssim -0\.5 must be >= 0"):
            Tr.main(["--alpha_ssim", "-0.5", "--phase", phase, "--synthetic", "16"])
        with pytest.raises(SystemExit, match=r"train\.py: --alpha_ssim 1\.0: \(--patch_size \* --scale\) = 2 \* 4 = 8 is smaller than the 11 x 11"):
            Tr.main(["--alpha_ssim", "1", "--phase", phase, "--patch_size", "2", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"--alpha_ssim 0\.25: .* = 5 \* 2 = 10 "):
        Tr.main(["--alpha_ssim", "0.25", "--patch_size", "5", "--scale", "2", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"--alpha_ssim nan must be >= 0"):
        Tr.main(["--alpha_ssim", "nan", "--synthetic", "16"])
    Tr.loss_terms_of(Tr.build_parser().parse_args(["--alpha_ssim", "1", "--patch_size", "3", "--scale", "4"]))   # 12: a window fits
    assert not calls


def test_trainer_term_is_off_by_default_and_refuses_a_negative_weight():
    from pesr_amd.step import Trainer
    assert not Trainer(None).use_ssim and not Trainer(None, alpha_ssim=0.0).use_ssim
    assert Trainer(None, alpha_ssim=0.25).use_ssim and Trainer(None, alpha_ssim=0.25).alpha_ssim == 0.25
    with pytest.raises(ValueError, match="alpha_ssim"):
        Trainer(None, alpha_ssim=-1.0)
