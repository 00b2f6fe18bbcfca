"""CPU: the JPEG round trip of docs/modes.md section 4l - the host-made tables (pesr_amd/jpeg.py), the float64 restatement
tests/jpeg_oracle.py against cases pinned by hand, against scipy's DCT, against its own stored outputs and against what Pillow's
libjpeg returned (tests/golden/gv17_jpeg.npz, made by tests/golden/make_golden_jpeg.py; the file is read, Pillow is not called) -
DegradationSpec's JPEG fields, the flag refusals of train.py / test.py, and the two new symbols of the C ABI."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest

import jpeg_oracle as JO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gv17_jpeg.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_jpeg_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def test_quant_tables_follow_the_ijg_quality_scale():
    from pesr_amd.jpeg import quant_tables
    for q in range(1, 101):                                     # product and restatement agree at every quality
        for a, b in zip(quant_tables(q), JO.quant_tables(q)):
            assert a.dtype == np.int64 and a.shape == (8, 8) and np.array_equal(a, b)
    L, C = quant_tables(50)
    assert np.array_equal(L, JO.LUMA) and np.array_equal(C, JO.CHROMA)                  # S = 100: the base tables
    assert L[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and C[0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99]
    assert all((t == 1).all() for t in quant_tables(100))
    L, C = quant_tables(1)                                      # S = 5000: 16 * 50 = 800 -> 255
    assert (L == 255).all() and (C == 255).all()
    # the switch of the formula: q = 49 -> S = 5000 // 49 = 102, q = 50 -> S = 200 - 100 = 100, q = 51 -> 98
    assert quant_tables(49)[0][0, :4].tolist() == [16, 11, 10, 16] and quant_tables(49)[0][7, 7] == 101 and quant_tables(49)[0][4, 5] == 111
    assert quant_tables(51)[0][0, :4].tolist() == [16, 11, 10, 16] and quant_tables(51)[0][7, 7] == 97 and quant_tables(51)[0][4, 5] == 107
    # q = 75 -> S = 50: (base * 50 + 50) // 100
    L, C = quant_tables(75)
    assert L[0].tolist() == [8, 6, 5, 8, 12, 20, 26, 31] and L[7].tolist() == [36, 46, 48, 49, 56, 50, 52, 50]
    assert C[0].tolist() == [9, 9, 12, 24, 50, 50, 50, 50] and C[3, 1] == 33
    # q = 10 -> S = 500, clamped at 255
    assert quant_tables(10)[0][0].tolist() == [80, 55, 50, 80, 120, 200, 255, 255]
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            quant_tables(bad)


def test_dct_table_is_the_orthonormal_dct_ii():
    import math
    from pesr_amd.jpeg import dct_table
    T = dct_table()
    assert T.dtype == np.float64 and T.shape == (8, 8) and np.array_equal(T, JO.dct_table())
    want = np.array([[0.5 * (math.sqrt(0.5) if u == 0 else 1.0) * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
    assert np.abs(T - want).max() <= 1e-15                        # (the direct formula rounds its angle, up to 105 pi / 16, first)
    assert np.abs(T @ T.T - np.eye(8)).max() <= 1e-15
    assert len(set(np.abs(T).reshape(-1).tolist())) == 7         # eight pinned values, 0.5 sqrt(0.5) twice


def test_restatement_without_roundings_is_scipys_dct():
    import scipy.fft
    b = np.random.default_rng(0).integers(0, 256, (3, 5, 8, 8)).astype(np.float64) - 128.0
    F = JO.fdct(b)
    assert np.abs(F - scipy.fft.dctn(b, axes=(-2, -1), norm="ortho")).max() <= 1e-9
    assert np.abs(JO.idct(F) - b).max() <= 1e-9
    assert np.abs(JO.idct(F) - scipy.fft.idctn(F, axes=(-2, -1), norm="ortho")).max() <= 1e-9
    # the whole plane coder without quantisation loss (Q = 1 keeps every integer coefficient ... of an already-integer plane)
    p = np.random.default_rng(1).integers(0, 256, (13, 21)).astype(np.float64)
    assert np.abs(JO.code_plane(p, np.full((8, 8), 1e-12), rounded=False) - p).max() <= 1e-9


# ---- cases pinned by hand ----------------------------------------------------------------------------------------------------------
def test_flat_grey_returns_itself_at_every_quality():
    img = np.full((19, 22, 3), 128, np.uint8)
    for q in (1, 10, 49, 50, 75, 100):
        for c420 in (True, False):
            assert np.array_equal(JO.jpeg(img, q, c420), img)


@pytest.mark.parametrize("v,q", [(200, 75), (77, 10), (131, 1), (90, 50), (255, 90), (0, 30)])
def test_flat_value_is_quantised_through_the_dc_term(v, q):
    """A flat grey image v: Y = v, Cb = Cr = 128; the only coefficient is the DC term 8 (v - 128), quantised by Q00."""
    Q00 = int(JO.quant_tables(q)[0][0, 0])
    dc = 8.0 * (v - 128) / Q00
    assert abs(abs(dc) - np.floor(abs(dc)) - 0.5) > 0.05                     # away from a rounding tie
    k = np.sign(dc) * np.floor(abs(dc) + 0.5)
    back = 128 + k * Q00 / 8.0
    assert abs(back - np.floor(back) - 0.5) > 0.05
    want = int(np.floor(min(max(back, 0.0), 255.0) + 0.5))
    for c420 in (True, False):
        out = JO.jpeg(np.full((16, 24, 3), v, np.uint8), q, c420)
        assert (out == want).all(), (out.min(), out.max(), want)


def test_checkerboard_hits_the_clamp_after_the_inverse_dct():
    y, x = np.mgrid[0:16, 0:16]
    img = np.repeat((((y + x) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    p = img[..., 0].astype(np.float64)
    raw = JO.code_plane(p, JO.quant_tables(50)[0], rounded=False)
    assert raw.min() < 0.0 and raw.max() > 255.0                            # the clamp matters
    out = JO.jpeg(img, 50, False)
    assert out.dtype == np.uint8 and out.min() == 0 and out.max() == 255
    # grey: Y is the image, the chroma planes are flat 128 - the red channel is the clamped, rounded Y plane
    assert np.array_equal(out[..., 0], JO.round8(raw).astype(np.uint8)) and np.array_equal(out[..., 0], out[..., 1])


def test_one_pixel_image():
    for rgb in ((0, 0, 0), (255, 255, 255), (200, 30, 90)):
        img = np.array(rgb, np.uint8).reshape(1, 1, 3)
        for c420 in (True, False):
            out = JO.jpeg(img, 100, c420)
            assert out.shape == (1, 1, 3) and np.abs(out.astype(int) - img.astype(int)).max() <= 2     # colour rounding only
            # the single pixel replicated to a block: equal to the flat 8 x 8 image's pixel
            for q in (10, 75):
                assert np.array_equal(JO.jpeg(img, q, c420)[0, 0], JO.jpeg(np.tile(img, (8, 8, 1)), q, c420)[0, 0])


# ---- structure -------------------------------------------------------------------------------------------------------------------
def test_blocks_are_independent_at_444():
    img = np.random.default_rng(3).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    swapped = img.copy()
    swapped[8:16, 0:8], swapped[16:24, 24:32] = img[16:24, 24:32], img[8:16, 0:8]
    a, b = JO.jpeg(img, 60, False), JO.jpeg(swapped, 60, False)
    want = a.copy()
    want[8:16, 0:8], want[16:24, 24:32] = a[16:24, 24:32], a[8:16, 0:8]
    assert np.array_equal(b, want) and not np.array_equal(a, b)


def test_a_window_does_not_depend_on_what_lies_outside_it():
    rng = np.random.default_rng(4)
    h, w, stride, off = 13, 21, 30, 7
    for c420 in (True, False):
        pools = [rng.integers(0, 256, off + 3 * stride * (h + 2), dtype=np.uint8) for _ in range(2)]
        win = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for p in pools:
            for y in range(h):
                p[off + 3 * stride * y:off + 3 * stride * y + 3 * w] = win[y].reshape(-1)
        a, b = (JO.jpeg_window(p, off, stride, h, w, 40, c420) for p in pools)
        assert np.array_equal(a, b) and np.array_equal(a, JO.jpeg(win, 40, c420))


def test_420_geometry():
    p = np.arange(15, dtype=np.float64).reshape(3, 5) * 4                    # odd sides: the last row and column are replicated
    d = JO.down420(p)
    assert d.shape == (2, 3) and d[0, 0] == (0 + 4 + 20 + 24) / 4 and d[1, 2] == p[2, 4] and d[0, 2] == (p[0, 4] + p[1, 4]) / 2
    assert JO.down420(np.array([[1.0, 2.0], [2.0, 1.0]]))[0, 0] == 2.0       # 1.5 rounds up
    c = np.array([[16.0, 32.0], [48.0, 64.0]])
    u = JO.up420(c, 4, 4)
    assert u[0, 0] == 16 and u[3, 3] == 64                                   # corners: every neighbour replicated
    assert u[1, 1] == (9 * 16 + 3 * 32 + 3 * 48 + 64) / 16 and u[2, 1] == (9 * 48 + 3 * 64 + 3 * 16 + 32) / 16
    assert u[0, 1] == (12 * 16 + 4 * 32) / 16


# ---- against Pillow's libjpeg, from the file -----------------------------------------------------------------------------------------
def _d(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def _golden_cases():
    g = np.load(GOLDEN)
    step = int(g["step"])
    for name in ("odd", "mcu"):
        for mode in ("444", "420"):
            for q in (int(v) for v in g["qualities"]):
                yield g, name, mode, q, (max(1, q - step), min(100, q + step))


def test_golden_file_is_what_the_issue_asks_for():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 512 * 1024
    assert g["qualities"].tolist() == [10, 50, 75, 90] and int(g["step"]) == 15
    assert any("Pillow" in str(v) for v in g["versions"]) and any("libjpeg" in str(v) for v in g["versions"])
    odd, mcu = g["odd_src"], g["mcu_src"]
    assert odd.shape[0] % 2 == 1 and odd.shape[1] % 2 == 1 and mcu.shape[0] % 16 == 0 and mcu.shape[1] % 16 == 0
    assert len(list(_golden_cases())) == 16


def test_restatement_equals_its_stored_outputs_bit_for_bit():
    for g, name, mode, q, _ in _golden_cases():
        assert np.array_equal(JO.jpeg(g[f"{name}_src"], q, mode == "420"), g[f"{name}_{mode}_ours_q{q}"]), (name, mode, q)


def test_definition_is_jpeg_witnessed_by_pillow():
    """(i) d(ours, pillow_q) / d(source, pillow_q) < 0.5: ours is far closer to the codec's result than the source is - a wrong table,
    quality scale, chroma order or level shift lands near 1 or above.  (ii) d(ours, pillow_q) < 0.5 * min over the neighbour qualities
    q - 15 and q + 15 (kept inside 1 .. 100) of d(ours, pillow_neighbour): the quality scale is IJG's."""
    for g, name, mode, q, (lo, hi) in _golden_cases():
        src, ours, pil = g[f"{name}_src"], g[f"{name}_{mode}_ours_q{q}"], g[f"{name}_{mode}_pillow_q{q}"]
        same = _d(ours, pil)
        r1 = same / _d(src, pil)
        near = min(_d(ours, g[f"{name}_{mode}_pillow_q{lo}"]), _d(ours, g[f"{name}_{mode}_pillow_q{hi}"]))
        print(f"{name} {mode} q={q}: d(ours, pillow) = {same:.4f} grey levels, (i) {r1:.4f}, (ii) {same / near:.4f} of the nearer neighbour ({lo}, {hi})")
        assert r1 < 0.5, (name, mode, q, r1)
        assert same < 0.5 * near, (name, mode, q, same, near)


# ---- DegradationSpec ---------------------------------------------------------------------------------------------------------------
def test_degradation_spec_without_jpeg_draws_what_it_drew_before():
    """The literals come from the DegradationSpec of the commit before the JPEG fields existed."""
    from pesr_amd.degrade import DegradationSpec
    r = random.Random(1234)
    spec = DegradationSpec(0.8, 3.2, True, 10.0)
    assert spec.jpeg_lo == 0 and spec.jpeg_hi == 0 and spec.jpeg_420 is True and tuple(spec) == (0.8, 3.2, True, 10.0)
    assert spec.draw(r) == (3.119488485661133, 1.822274189042734, 0.023535147300645414, 9.109759624491241, 14886566920684039889)
    assert spec.draw(r) == (2.1973461753414782, 1.7384066623562435, 0.2636997167867366, 7.664809327917963, 321490749937914057)
    assert r.getrandbits(32) == 132345184                                    # the stream is where it was
    r = random.Random(1234)
    spec = DegradationSpec(0.4, 1.6)
    assert spec.draw(r) == (1.5597442428305666, 1.5597442428305666, 0.0, 0.0, 2155511622373988895)
    assert spec.draw(r) == (0.40898976407030463, 0.40898976407030463, 0.0, 0.0, 17386697504169769072)
    assert r.getrandbits(32) == 4034129617
    assert spec.check() is spec


def test_degradation_spec_with_jpeg_appends_the_quality():
    from pesr_amd.degrade import DegradationSpec
    off, on = DegradationSpec(0.8, 3.2, True, 10.0), DegradationSpec(0.8, 3.2, True, 10.0, 30, 95, False)
    a, b = random.Random(7), random.Random(7)
    seen = set()
    for _ in range(200):
        x, y = off.draw(a), on.draw(b)
        assert len(y) == 6 and y[:5] == x and isinstance(y[5], int) and 30 <= y[5] <= 95
        seen.add(y[5])
        assert a.randint(30, 95) == y[5]                                     # drawn after q, by randint, from the same stream
    assert len(seen) > 30
    assert DegradationSpec(1.0, 2.0, jpeg_lo=40, jpeg_hi=40).draw(random.Random(0))[5] == 40
    assert on.check() is on
    for lo, hi in ((0, 50), (50, 40), (1, 101), (-5, 50), (60, 0)):
        with pytest.raises(SystemExit, match="1 <= LO <= HI <= 100"):
            DegradationSpec(1.0, 2.0, False, 0.0, lo, hi).check("x")


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_train_refuses_jpeg_quality_without_its_companions():
    Tm = _load("train")
    full = ["--degradation", "classical", "--lr_from_hr", "true", "--gpu_pipeline", "true", "--jpeg_quality", "30,95"]
    spec = Tm.degradation_spec(Tm.build_parser().parse_args(full))
    assert (spec.jpeg_lo, spec.jpeg_hi, spec.jpeg_420) == (30, 95, True)
    assert Tm.degradation_spec(Tm.build_parser().parse_args(full + ["--jpeg_chroma", "444"])).jpeg_420 is False
    plain = Tm.degradation_spec(Tm.build_parser().parse_args(full[:6]))
    assert (plain.jpeg_lo, plain.jpeg_hi) == (0, 0) and Tm.degradation_spec(Tm.build_parser().parse_args([])) is None
    for argv in (["--jpeg_quality", "30,95"],                                                               # bicubic
                 ["--jpeg_quality", "30,95", "--lr_from_hr", "true", "--gpu_pipeline", "true"],
                 ["--jpeg_quality", "30,95", "--degradation", "classical", "--gpu_pipeline", "true"],
                 ["--jpeg_quality", "30,95", "--degradation", "classical", "--lr_from_hr", "true"],
                 full + ["--synthetic", "8"]):
        with pytest.raises(SystemExit) as e:
            Tm.degradation_spec(Tm.build_parser().parse_args(argv))
        msg = str(e.value)
        assert "--lr_from_hr true" in msg and "--gpu_pipeline true" in msg and "--degradation classical" in msg, msg
    for bad in ("50", "0,50", "60,40", "10,101", "a,b", "10,20,30"):
        with pytest.raises(SystemExit, match="--jpeg_quality"):
            Tm.degradation_spec(Tm.build_parser().parse_args(full[:6] + ["--jpeg_quality", bad]))
    with pytest.raises(SystemExit):
        Tm.build_parser().parse_args(full + ["--jpeg_chroma", "422"])


def test_test_refuses_jpeg_quality_without_from_hr():
    T = _load("test")
    p = T.build_parser()
    assert T.jpeg_quality(p.parse_args([])) == 0
    assert T.jpeg_quality(p.parse_args(["--from_hr", "true", "--jpeg_quality", "30"])) == 30
    assert T.jpeg_quality(p.parse_args(["--from_hr", "true", "--degradation", "classical", "--jpeg_quality", "100"])) == 100
    with pytest.raises(SystemExit, match="--jpeg_quality .* needs --from_hr true"):
        T.jpeg_quality(p.parse_args(["--jpeg_quality", "30"]))
    for bad in ("0", "101", "30,40", "x"):
        with pytest.raises(SystemExit, match="--jpeg_quality"):
            T.jpeg_quality(p.parse_args(["--from_hr", "true", "--jpeg_quality", bad]))
    with pytest.raises(SystemExit):
        p.parse_args(["--jpeg_chroma", "422"])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_jpeg_symbols_and_the_host_side_workspace_size():
    """pesr_jpeg_workspace_bytes is host-only code: the sum over the entries, 0 for descriptors the launch would refuse."""
    from pesr_amd import _lib
    from pesr_amd.jpeg import DESC_WORDS, entry_bytes
    L = _lib.lib()
    assert "pesr_jpeg_u8" in _lib.SIGNATURES and hasattr(L, "pesr_jpeg_u8") and L.pesr_abi_version() == 20

    def size(rows, chroma, n=None):
        d = np.array(rows, dtype=np.int64).reshape(-1, DESC_WORDS)
        return L.pesr_jpeg_workspace_bytes(d.ctypes.data_as(ctypes.c_void_p), len(d) if n is None else n, chroma)

    one = (0, 20, 0, 20, 15, 17, 75, 0)
    assert size([one], 420) == 15 * 17 + 2 * 8 * 9 == entry_bytes(15, 17, True)
    assert size([one], 444) == 3 * 15 * 17 == entry_bytes(15, 17, False)
    two = (5, 40, 900, 33, 1, 33, 1, 15 * 17 + 2 * 8 * 9)
    assert size([one, two], 420) == 15 * 17 + 2 * 8 * 9 + 33 + 2 * 17
    assert size([one, two], 444) == 0                                        # the second offset is not the running sum at 4:4:4
    assert size([one], 422) == 0 and size([one], 420, n=0) == 0
    for word, bad in ((4, 0), (5, 0), (6, 0), (6, 101), (1, 16), (3, 16), (0, -1), (2, -1), (7, 8)):
        row = list(one)
        row[word] = bad
        assert size([row], 420) == 0, (word, bad)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        import torch
        from pesr_amd.jpeg import jpeg_u8
        jpeg_u8(torch.zeros(8, 8, 3, dtype=torch.uint8), 50)
