"""CPU: the definition of the bicubic resize (docs/modes.md section 4f) - host weights of pesr_amd.resize against the float64
restatement tests/resize_oracle.py, the restatement against torch's antialiased bicubic (interior) and against cases written out by
hand (border, rounding), the committed fixture GV14, FolderSRDataset(lr_from_hr=...) and the new flags of train.py / test.py."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_oracle as RO
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_host_weights_equal_the_restatement(s, up):
    from pesr_amd.resize import down_offsets, resize_weights, up_first_tap
    w, want = resize_weights(s, up), RO.weights(s, up)
    assert w.dtype == np.float64 and w.shape == want.shape == ((s, 4) if up else ({2: 8, 3: 11, 4: 16}[s],))
    assert np.array_equal(w, want) and w.size <= 16
    if up:
        assert [up_first_tap(s, p) for p in range(s)] == [RO.up_taps(s, p)[0] for p in range(s)]
    else:
        assert down_offsets(s) == RO.down_taps(s)[0]
    for row in w.reshape(-1, w.shape[-1]):
        total = 0.0
        for v in row:
            total = total + v
        assert abs(total - 1.0) <= np.spacing(1.0)
    if s != 3:       # dyadic: every product w * (0..255) and every partial sum is exact in float64 - the reason ties are exact
        assert np.array_equal(w * 2.0 ** 16, np.round(w * 2.0 ** 16))
    elif not up:     # the two taps at distance exactly 1 from the centre (in output pixels) weigh exactly zero and are kept
        assert w[2] == 0.0 and w[8] == 0.0 and np.count_nonzero(w) == 9


def test_unsupported_factor_and_cpu_tensor_are_errors():
    from pesr_amd import _lib
    from pesr_amd.resize import imresize_pool_u8, imresize_u8, resize_weights
    with pytest.raises(ValueError):
        resize_weights(5, False)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), 2)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_pool_u8(torch.zeros(48, dtype=torch.uint8), [0], [(4, 4)], 2)


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_unrounded_restatement_equals_torch_antialiased_bicubic_on_the_interior(s, up):
    """An independent implementation pins kernel, coordinates and antialiasing: away from the border (further than 2s input pixels
    on the way down, 2 on the way up) the float64 result without the two roundings is torch's bicubic with antialias=True.  (torch
    without antialias uses a = -0.75; at the border torch truncates the window where MATLAB reflects.)"""
    h, w = 12 * s + (0 if not up else 1), 15 * s
    img = np.random.default_rng(s + 10 * up).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = RO.imresize(img, s, up, rounded=False)
    x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    size = (h * s, w * s) if up else (h // s, w // s)
    ref = F.interpolate(x, size=size, mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    assert got.shape == ref.shape
    m = 2 * s + 1 if up else 3                       # in output pixels
    err = np.abs(got - ref)
    print(f"x{s} {'up' if up else 'down'}: interior max |restatement - torch| = {err[m:-m, m:-m].max():.3e}, border {err.max():.3e}")
    assert err[m:-m, m:-m].max() <= 1e-9
    assert err.max() > 1.0                            # and the border rule is NOT torch's


def _round_half_up(fr):
    return int((fr + Fraction(1, 2)).__floor__())


def _clamp(fr):
    return min(max(fr, Fraction(0)), Fraction(255))


def test_one_dimensional_cases_written_out_x2():
    """x2 weights are k(-7/4 .. 7/4) / 2 = (-3, -9, 29, 111, 111, 29, -9, -3) / 256 (down) and, per phase, k / 1 =
    (-3, 29, 111, -9) / 128 and (-9, 111, 29, -3) / 128 (up).  The reflected indices are listed by hand."""
    assert np.array_equal(RO.weights(2, False) * 256, [-3, -9, 29, 111, 111, 29, -9, -3])
    assert np.array_equal(RO.weights(2, True) * 128, [[-3, 29, 111, -9], [-9, 111, 29, -3]])
    v = [13, 250, 7, 131]
    # down, n = 4: output 0 reads -3 .. 4, output 1 reads -1 .. 6   ( ... 2 1 0 | 0 1 2 3 | 3 2 1 ... )
    idx = [[2, 1, 0, 0, 1, 2, 3, 3], [0, 0, 1, 2, 3, 3, 2, 1]]
    wd = [-3, -9, 29, 111, 111, 29, -9, -3]
    want = [_round_half_up(_clamp(sum(Fraction(w * v[j], 256) for w, j in zip(wd, ix)))) for ix in idx]
    col = np.array(v, dtype=np.float64).reshape(4, 1)
    assert RO.resize_axis0(col, 2, False)[:, 0].tolist() == want
    # up, n = 2: outputs 0 .. 3 read -2 .. 1, -1 .. 2, -1 .. 2, 0 .. 3   ( ... 1 0 | 0 1 | 1 0 ... )
    v2 = [200, 31]
    idx = [[1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 1, 1, 0]]
    wu = [[-3, 29, 111, -9], [-9, 111, 29, -3]]
    want = [_round_half_up(_clamp(sum(Fraction(w * v2[j], 128) for w, j in zip(wu[o % 2], idx[o])))) for o in range(4)]
    col = np.array(v2, dtype=np.float64).reshape(2, 1)
    assert RO.resize_axis0(col, 2, True)[:, 0].tolist() == want


def _exact_1d(v, s, up):
    """Exact rational arithmetic, written from the definition's sentences: per-output centre, all taps inside the support."""
    n = len(v)

    def k(x):
        x = abs(x)
        if x <= 1:
            return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
        if x <= 2:
            return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
        return Fraction(0)

    def refl(j):
        while j < 0 or j >= n:
            j = -j - 1 if j < 0 else 2 * n - 1 - j
        return j

    out = []
    for o in range(n * s if up else n // s):
        if up:
            c = Fraction(o // s) + Fraction(2 * (o % s) + 1 - s, 2 * s)
            taps = [(j, k(j - c)) for j in range(c.__floor__() - 1, c.__floor__() + 3)]
        else:
            c = Fraction(s * o) + Fraction(s - 1, 2)
            taps = [(j, k((j - c) / s)) for j in range(s * o - 3 * s, s * o + 3 * s + 1) if abs(j - c) < 2 * s]
        total = sum(w for _, w in taps)
        out.append(_round_half_up(_clamp(sum(w * v[refl(j)] for j, w in taps) / total)))
    return out


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_one_dimensional_cases_against_exact_arithmetic(s, up):
    rng = np.random.default_rng(77 + s)
    for n in ([1, 2, 5] if up else [s, 2 * s, 7 * s]):      # n = s: one output, every tap but s of them reflected
        v = rng.integers(0, 256, n).tolist()
        got = RO.resize_axis0(np.array(v, dtype=np.float64).reshape(n, 1), s, up)[:, 0].tolist()
        assert got == _exact_1d(v, s, up), (s, up, n)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_constant_image_stays_constant(s):
    for value in (0, 1, 128, 254, 255):
        img = np.full((2 * s, 3 * s, 3), value, np.uint8)
        assert (RO.imresize(img, s, False) == value).all() and RO.imresize(img, s, False).shape == (2, 3, 3)
        assert (RO.imresize(img, s, True) == value).all() and RO.imresize(img, s, True).shape == (2 * s * s, 3 * s * s, 3)


def test_ties_round_half_up_and_the_intermediate_image_is_rounded():
    """A 2 x 2 image reduced by 2: every tap is a reflection of the two pixels of its column (row), each with total weight
    exactly 1/2, so a pass is (a + b) / 2 - exact ties on demand."""
    def img(a, b, c, d):
        return np.array([[[a] * 3, [b] * 3], [[c] * 3, [d] * 3]], dtype=np.uint8)
    # columns (0 + 1) / 2 = 0.5 -> 1 (half up; half-to-even would give 0), then (1 + 1) / 2 = 1
    assert RO.imresize(img(0, 0, 1, 1), 2).tolist() == [[[1, 1, 1]]]
    assert np.round(0.5) == 0.0
    # (2 + 3) / 2 = 2.5 -> 3 (half-to-even: 2)
    assert RO.imresize(img(2, 2, 3, 3), 2).tolist() == [[[3, 3, 3]]]
    # rounding BETWEEN the passes: columns 0.5 -> 1 and 0 -> 0, then (1 + 0) / 2 = 0.5 -> 1; in one go 0.25 -> 0
    assert RO.imresize(img(0, 0, 1, 0), 2).tolist() == [[[1, 1, 1]]]
    assert RO.imresize(img(0, 0, 1, 0), 2, rounded=False).tolist() == [[[0.25, 0.25, 0.25]]]
    # the ramp: more than half of the first pass's values are exact ties at x2 and x4, none at x3
    y, x = np.mgrid[0:48, 0:48]
    ramp = ((2 * x + y) % 256).astype(np.float64)[:, :, None]
    for s, lo, hi in ((2, 0.4, 1.0), (4, 0.4, 1.0), (3, 0.0, 0.0)):
        v = RO.resize_axis0(ramp, s, False, rounded=False)
        share = float(np.mean(v - np.floor(v) == 0.5))
        assert lo <= share <= hi, (s, share)


def test_fixture_gv14_pins_the_restatement():
    g = load_golden("gv14_imresize")
    names = sorted(k[:-3] for k in g.files if k.endswith("_in"))
    assert names == ["ragged", "ramp", "random"]
    for name in names:
        img = g[f"{name}_in"]
        for s in (2, 3, 4):
            assert np.array_equal(RO.imresize(RO.modcrop(img, s), s, False), g[f"{name}_down{s}"]), (name, s, "down")
            assert np.array_equal(RO.imresize(img, s, True), g[f"{name}_up{s}"]), (name, s, "up")
    assert g["ragged_in"].shape == (17, 14, 3) and g["ragged_down3"].shape == (5, 4, 3) and g["ragged_down4"].shape == (4, 3, 3)


def test_modcrop():
    from pesr_amd.resize import modcrop
    a = np.arange(7 * 11 * 3, dtype=np.uint8).reshape(7, 11, 3)
    for s in (2, 3, 4):
        c = modcrop(a, s)
        assert c.shape == (7 - 7 % s, 11 - 11 % s, 3) and np.array_equal(c, a[:c.shape[0], :c.shape[1]])
        assert np.array_equal(c, RO.modcrop(a, s))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_folder_dataset_from_hr_alone(tmp_path, s):
    import random
    from PIL import Image
    D = _load("data")
    rng = np.random.RandomState(s)
    root = tmp_path / "hr_only"
    (root / "HR").mkdir(parents=True)
    hrs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((8 * s + 1, 9 * s + s - 1), (7 * s, 8 * s), (10 * s, 7 * s + 1))]
    for i, im in enumerate(hrs):
        Image.fromarray(im).save(root / "HR" / f"{i}.png")
    calls = []

    def lr_from_hr(hr):
        calls.append(hr.shape)
        return RO.imresize(hr, s, False)

    ds = D.FolderSRDataset(str(root), None, 2, False, scale=s, lr_from_hr=lr_from_hr)
    assert len(ds) == 6 and len(calls) == 3                              # the LR images are made once, at construction
    assert calls[0] == (8 * s, 9 * s, 3)                                 # ... from the mod-cropped image
    for i, im in enumerate(hrs):
        lr, hr = ds[i]
        crop = RO.modcrop(im, s)
        assert torch.equal(hr, D.to_tensor(crop)) and torch.equal(lr, D.to_tensor(RO.imresize(crop, s, False)))
        assert torch.equal(ds[i + 3][0], lr)
    assert len(calls) == 3
    assert len(D.FolderSRDataset(str(root), None, 1, False, fixed_length=2, scale=s, lr_from_hr=lr_from_hr)) == 2
    # random crops stay aligned: the HR patch is the mod-cropped image at s*y, s*x of where the LR patch sits
    P = 5
    ds = D.FolderSRDataset(str(root), P, 1, False, scale=s, lr_from_hr=lr_from_hr)
    random.seed(4)
    for i in range(3):
        lr, hr = ds[i]
        assert lr.shape == (3, P, P) and hr.shape == (3, s * P, s * P)
        full_lr = RO.imresize(RO.modcrop(hrs[i], s), s, False)
        where = [(y, x) for y in range(full_lr.shape[0] - P + 1) for x in range(full_lr.shape[1] - P + 1)
                 if torch.equal(lr, D.to_tensor(full_lr[y:y + P, x:x + P]))]
        assert any(torch.equal(hr, D.to_tensor(hrs[i][s * y:s * (y + P), s * x:s * (x + P)])) for y, x in where)
    # without the callable nothing changes: LR/ decides the file list, and an HR-only folder is empty
    assert len(D.FolderSRDataset(str(root), None, 1, False, scale=s)) == 0
    both = tmp_path / "both"
    (both / "HR").mkdir(parents=True), (both / "LR").mkdir()
    lr_img = rng.randint(0, 256, (6, 5, 3)).astype(np.uint8)
    hr_img = rng.randint(0, 256, (6 * s, 5 * s, 3)).astype(np.uint8)
    Image.fromarray(lr_img).save(both / "LR" / "a.png"), Image.fromarray(hr_img).save(both / "HR" / "a.png")
    Image.fromarray(hr_img).save(both / "HR" / "no_lr_partner.png")
    ds = D.FolderSRDataset(str(both), None, 1, False, scale=s)
    assert len(ds) == 1
    lr, hr = ds[0]
    assert torch.equal(lr, D.to_tensor(lr_img)) and torch.equal(hr, D.to_tensor(hr_img))      # the stored LR, not a resize


def test_new_flags_exist_and_default_to_false():
    Tr, Te = _load("train"), _load("test")
    a = Tr.build_parser().parse_args([])
    assert a.lr_from_hr is False and a.gpu_pipeline is False
    assert Tr.build_parser().parse_args(["--lr_from_hr", "true"]).lr_from_hr is True
    b = Te.build_parser().parse_args([])
    assert b.from_hr is False
    assert Te.build_parser().parse_args(["--from_hr", "true"]).from_hr is True
    assert Te.build_parser().parse_args(["--from_hr", "false"]).from_hr is False
