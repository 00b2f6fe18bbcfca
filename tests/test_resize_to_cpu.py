"""CPU: the any-size resize of docs/modes.md section 4m - its restatement tests/resize_to_oracle.py against section 4f's, against hand
cases, against exact rational arithmetic and against torch's antialiased interpolate; the host-side table maker of
pesr_amd/resize.py against the restatement; DegradationSpec's resize jitter.  No GPU is involved."""
import math
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import resize_oracle as RO
import resize_to_oracle as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gv18_resize_to.npz")


def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- where 4m overlaps 4f -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_integer_factors_with_bicubic_are_section_4f_bit_for_bit(s):
    img = _img(24, 36, s)
    ramp = (np.arange(24 * 36 * 3).reshape(24, 36, 3) % 256).astype(np.uint8)         # the tie-heavy integer ramp
    for a in (img, ramp):
        assert np.array_equal(RT.resize(a, (24 // s, 36 // s)), RO.imresize(a, s, up=False))
        assert np.array_equal(RT.resize(a, (24 * s, 36 * s)), RO.imresize(a, s, up=True))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_integer_factors_give_section_4fs_offsets_and_arguments(s):
    n = 5
    for o, (js, _) in enumerate(RT.taps(s * n, n, "bicubic")):                       # down: taps s*o + t, argument (2t - (s-1)) / (2s)
        assert [j - s * o for j in js] == [t for t in range(-3 * s, 3 * s) if abs(2 * t - (s - 1)) < 4 * s]
        for j in js:
            N, t = (2 * j + 1) * n - (2 * o + 1) * s * n, j - s * o
            assert N / (2 * s * n) == (2 * t - (s - 1)) / (2 * s)
    for o, (js, _) in enumerate(RT.taps(n, s * n, "bicubic")):                       # up: output s*q + p, argument (2s(j-q) - (2p+1-s)) / (2s)
        q, p = divmod(o, s)
        assert js[0] - q == (-2 if 2 * p + 1 - s < 0 else -1)
        assert len(js) == 4 or (len(js) == 3 and 2 * p + 1 == s)            # the centred phase of x3: 4f's fourth tap sits at k(2) = 0, outside |N| < 4M
        for j in js:
            assert ((2 * j + 1) * s * n - (2 * o + 1) * n) / (2 * s * n) == (2 * s * (j - q) - (2 * p + 1 - s)) / (2 * s)


@pytest.mark.parametrize("method", RT.METHODS)
def test_equal_size_is_the_identity(method):
    for h, w in ((1, 1), (7, 5), (16, 33)):
        img = _img(h, w, h)
        assert np.array_equal(RT.resize(img, (h, w), method), img)


# ---- hand cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_box_by_an_integer_is_the_mean_down_and_a_repeat_up(s):
    col = _img(8 * s, 1, s)
    mean = col.astype(np.int64).reshape(8, s, 1, 3).sum(axis=1)
    assert np.array_equal(RT.resize(col, (8, 1), "box"), ((2 * mean + s) // (2 * s)).astype(np.uint8))      # floor(mean + 1/2), exactly
    small = _img(3, 5, s)
    assert np.array_equal(RT.resize(small, (3 * s, 5 * s), "box"), small.repeat(s, axis=0).repeat(s, axis=1))


def test_bilinear_x2_down_has_weights_1_3_3_1_over_8():
    for o, (js, ws) in enumerate(RT.taps(12, 6, "bilinear")):
        assert js == [2 * o - 1, 2 * o, 2 * o + 1, 2 * o + 2] and ws == [0.125, 0.375, 0.375, 0.125]


@pytest.mark.parametrize("method", RT.METHODS)
def test_single_output_pixel_and_single_input_pixel(method):
    img = _img(5, 7, 9)
    one = RT.resize(img, (1, 1), method)
    assert one.shape == (1, 1, 3)
    if method == "box":                                         # n_out = 1: -M <= N < M takes every input once: the mean of the means
        mid = (2 * img.astype(np.int64).sum(axis=0) + 5) // 10                      # floor(mean + 1/2) of the 5 rows, exactly
        assert np.array_equal(one[0, 0], (2 * mid.sum(axis=0) + 7) // 14) and RT.taps(5, 1, "box")[0][0] == [0, 1, 2, 3, 4]
    px = _img(1, 1, 4)
    assert np.array_equal(RT.resize(px, (5, 3), method), np.broadcast_to(px, (5, 3, 3)))


# ---- exact rational arithmetic -------------------------------------------------------------------------------------------------------
def _exact_kernel(method, x):
    x = abs(x)
    if method == "bicubic":
        if x <= 1:
            return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
        if x <= 2:
            return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
        return Fraction(0)
    if method == "bilinear":
        return 1 - x if x <= 1 else Fraction(0)
    return Fraction(1)


def _exact_1d(v, n_out, method):
    """The definition on a list of integers in exact rationals, rounded once."""
    n_in, M, out = len(v), max(len(v), n_out), []
    for o in range(n_out):
        num = den = Fraction(0)
        for j in range(-40 * 8, n_in + 40 * 8):
            N = (2 * j + 1) * n_out - (2 * o + 1) * n_in
            if RT.inside(method, N, M):
                w = _exact_kernel(method, Fraction(N, 2 * M))
                num += w * int(v[RT.reflect(j, n_in)])
                den += w
        out.append(min(255, max(0, math.floor(num / den + Fraction(1, 2)))))
    return out


@pytest.mark.parametrize("method", RT.METHODS)
def test_one_axis_equals_exact_rational_arithmetic(method):
    rng = np.random.default_rng(12)
    for n_in, n_out in ((7, 3), (10, 7), (5, 13), (16, 2), (2, 16), (9, 9), (11, 4), (4, 11), (33, 5), (1, 6), (6, 1)):
        v = rng.integers(0, 256, n_in)
        col = np.repeat(v.astype(np.uint8)[:, None, None], 3, axis=2)                 # n_in x 1 image; the 1 -> 1 width pass is the identity
        got = RT.resize(col, (n_out, 1), method)[:, 0, 0].tolist()
        assert got == _exact_1d(v, n_out, method), (method, n_in, n_out)
        row = col.transpose(1, 0, 2)
        assert RT.resize(row, (1, n_out), method)[0, :, 0].tolist() == got


# ---- torch as the outside witness of bicubic and bilinear ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size", [(33, 61), (24, 72), (61, 33)])
def test_unrounded_interior_equals_torchs_antialiased_interpolate(method, size):
    import torch
    img = _img(48, 48, 21).astype(np.float64)
    ho, wo = size
    ours = RT.resize_axis0(RT.resize_axis0(img, ho, method).transpose(1, 0, 2), wo, method).transpose(1, 0, 2)      # no rounding in between
    t = torch.from_numpy(img).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(t, size=size, mode=method, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    rows = [o for o, (js, _) in enumerate(RT.taps(48, ho, method)) if js[0] >= 0 and js[-1] < 48]       # no reflected tap
    cols = [o for o, (js, _) in enumerate(RT.taps(48, wo, method)) if js[0] >= 0 and js[-1] < 48]
    assert len(rows) >= ho - 8 and len(cols) >= wo - 8 and len(rows) < ho and len(cols) < wo
    d = np.abs(ours - ref)[np.ix_(rows, cols)].max()
    print(f"{method} 48 x 48 -> {ho} x {wo}: interior max |ours - torch| = {d:.3g}")
    assert d <= 1e-9


# ---- the limits, and the product's table maker ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RT.METHODS)
def test_tap_count_stays_within_32_at_the_limits(method):
    from pesr_amd.resize import MAX_TAPS, resize_table
    assert MAX_TAPS == 32
    worst = 0
    for n in range(1, 41):
        for n_in, n_out in ((8 * n, n), (8 * n - 1, n), (8 * n - 7, n), (n, 8 * n), (n, 8 * n - 3), (7 * n + 3, n)):
            if n_in >= 1 and n_out >= 1 and n_in <= 8 * n_out and n_out <= 8 * n_in:
                worst = max(worst, resize_table(n_in, n_out, method)[1].shape[1], max(len(js) for js, _ in RT.taps(n_in, n_out, method)))
    assert worst <= 32 and (method != "bicubic" or worst == 32)


@pytest.mark.parametrize("method", RT.METHODS)
def test_table_maker_equals_the_restatement(method):
    from pesr_amd.resize import METHODS, resize_table
    assert METHODS == RT.METHODS == ("bicubic", "bilinear", "box")
    for n_in, n_out in ((1, 1), (1, 8), (8, 1), (9, 4), (13, 29), (345, 100), (100, 345), (48, 33), (48, 6), (6, 48), (48, 18), (37, 37)):
        first, w = resize_table(n_in, n_out, method)
        rows = RT.taps(n_in, n_out, method)
        assert first.dtype == np.int64 and w.dtype == np.float64 and first.shape == (n_out,) and w.shape[0] == n_out
        assert w.shape[1] == max(len(js) for js, _ in rows)
        for o, (js, ws) in enumerate(rows):
            assert first[o] == js[0] and w[o, :len(ws)].tolist() == ws and not w[o, len(ws):].any(), (n_in, n_out, o)
    for bad in ((0, 1), (1, 0), (9, 1), (1, 9), (17, 2)):
        with pytest.raises(ValueError):
            resize_table(bad[0], bad[1], method)
    with pytest.raises(ValueError):
        resize_table(4, 4, "lanczos")


def test_no_cpu_fallback_and_the_new_symbol():
    import torch
    from pesr_amd import _lib
    from pesr_amd.resize import imresize_to_pool_u8, imresize_to_u8
    assert "pesr_resize_to_u8_pass" in _lib.SIGNATURES
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_to_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), (3, 5))
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_to_pool_u8(torch.zeros(48, dtype=torch.uint8), [0], [(4, 4)], [(3, 5)], "box")


# ---- golden file ----------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_its_stored_outputs_bit_for_bit():
    g = np.load(GOLDEN)
    img, (sigma, q) = g["src"], g["noise"]
    assert img.shape == (37, 53, 3) and len(g.files) == 4 + 3 * (len(g["sizes"]) + 1) + 3 * len(g["jitter"])
    for m in RT.METHODS:
        for ho, wo in g["sizes"]:
            assert np.array_equal(RT.resize(img, (int(ho), int(wo)), m), g[f"{m}_{ho}x{wo}"]), (m, ho, wo)
        assert np.array_equal(RT.resize(img, tuple(int(v) for v in g["sizes"][0]), m, float(sigma), int(q)), g[f"{m}_noisy"])
        assert not np.array_equal(g[f"{m}_noisy"], g["{}_{}x{}".format(m, *g["sizes"][0])])
    for r in g["jitter"]:
        for m1 in range(3):
            assert np.array_equal(RT.jitter(img, float(r), m1, (m1 + 1) % 3, float(sigma), int(q)), g[f"jitter_{r}_{m1}"])


# ---- DegradationSpec ----------------------------------------------------------------------------------------------------------------
PARENT_DRAWS = (    # DegradationSpec(*args).draw(random.Random(7)) on the commit before the resize jitter
    ((0.8, 3.2), (1.57719863559959, 1.57719863559959, 0.0, 0.0, 7283207964119141687)),
    ((0.8, 3.2, True, 25.0), (1.57719863559959, 0.9172397721554482, 2.0449709584703477, 1.810907166688569, 1736392818365009963)),
    ((0.8, 3.2, False, 10.0, 30, 95), (1.57719863559959, 1.57719863559959, 0.0, 1.5084917392450192, 890727360438182992, 39)),
    ((0.5, 2.0, True, 0.0, 10, 10, False), (0.9857491472497435, 0.573274857597155, 2.0449709584703477, 0.0, 15149836622520594227, 10)),
)


def test_spec_without_jitter_draws_what_it_drew_before():
    from pesr_amd.degrade import DegradationSpec
    for args, want in PARENT_DRAWS:
        for spec in (DegradationSpec(*args), DegradationSpec(*(args + (False, 0.0, 0, 0, True)[len(args) - 2:]), 0.0, 0.0)):
            rng = random.Random(7)
            assert spec.draw(rng) == want and len(spec.fields()) == len(want)
            ref = random.Random(7)
            DegradationSpec(*args).draw(ref)
            assert rng.getstate() == ref.getstate()                                # consumed exactly the same numbers
            assert tuple(spec) == (tuple(args) + (False, 0.0))[:4] and spec.jitter_lo == 0.0 and spec.jitter_hi == 0.0


def test_spec_with_jitter_appends_r_and_two_filters_after_everything_else():
    from pesr_amd.degrade import DegradationSpec
    for args, want in PARENT_DRAWS:
        full = args + (False, 0.0, 0, 0, True)[len(args) - 2:]
        spec = DegradationSpec(*full, 0.5, 2.0)
        rng, ref = random.Random(7), random.Random(7)
        got = spec.draw(rng)
        assert got[:len(want)] == want == DegradationSpec(*args).draw(ref)
        tail = (ref.uniform(0.5, 2.0), ref.randrange(3), ref.randrange(3))
        assert got[len(want):] == tail and rng.getstate() == ref.getstate()
        names = spec.fields()
        assert names[:5] == ("sigma1", "sigma2", "theta", "sigma_n", "q") and names[-3:] == ("jitter_r", "jitter_m1", "jitter_m2")
        assert ("jpeg_quality" in names) == (len(want) == 6) and len(names) == len(got)
        d = spec.named(got)
        assert (d["jitter_r"], d["jitter_m1"], d["jitter_m2"]) == tail and d["q"] == want[4]
        assert tuple(spec) == tuple(full[:4]) and len(spec) == 4                     # as a tuple: the four blur and noise values
        assert "0.5, 2.0" in repr(spec)


def test_check_refuses_a_jitter_range_outside_an_eighth_to_eight():
    from pesr_amd.degrade import DegradationSpec
    for lo, hi in ((0.125, 8), (1, 1), (0.5, 2.0), (0, 0)):
        DegradationSpec(1.0, 2.0, jitter_lo=lo, jitter_hi=hi).check()
    for lo, hi in ((0.1, 2), (0.5, 8.5), (2, 0.5), (0, 2), (-1, 2), (float("nan"), 2), (0.5, float("nan")), (0.5, float("inf")), (0.5, 0)):
        with pytest.raises(SystemExit, match="resize-jitter range"):
            DegradationSpec(1.0, 2.0, jitter_lo=lo, jitter_hi=hi).check("who")


def test_intermediate_size_at_its_clamps():
    from pesr_amd.degrade import jitter_size
    assert [jitter_size(48, r) for r in (0.125, 0.37, 0.5, 1.0, 1.6, 8.0)] == [6, 18, 24, 48, 77, 384]
    assert jitter_size(10, 0.125) == 2                      # floor(1.25 + 0.5) = 1 would be beyond 8:1: ceil(10 / 8)
    assert jitter_size(9, 0.125) == 2 and jitter_size(8, 0.125) == 1 and jitter_size(1, 0.125) == 1 and jitter_size(1, 0.3) == 1
    assert jitter_size(5, 0.5) == 3                         # 2.5 rounds half up
    assert jitter_size(3, 7.9) == 24 and jitter_size(3, 8.0) == 24 and jitter_size(1, 8.0) == 8
    for n in range(1, 60):
        for r in (0.125, 0.13, 0.3, 0.99, 1.01, 3.3, 7.99, 8.0):
            Q = jitter_size(n, r)
            assert Q == RT.jitter_size(n, r) and 1 <= Q and n <= 8 * Q and Q <= 8 * n
