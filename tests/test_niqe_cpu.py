"""CPU: the definition of NIQE (docs/modes.md section 4k) - the float64 restatement tests/niqe_oracle.py against closed forms and
independent formulations (scipy, torch, tests/resize_oracle.py), the host half of the product (pesr_amd/niqe.py: numpy route, AGGD
fits, features, model files, fitting, score) against the restatement, a golden file, and the refusals of the C ABI, test.py and
train.py."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import niqe_cases as C
import niqe_oracle as NO
import resize_oracle as RO
from pesr_amd import niqe as NQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gv16_niqe.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_niqe_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _smooth_edge(seed, h=96, w=120):
    """A smooth image with a few rectangular edges and a little grain, [3, h, w], uint8-valued."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 100 + 40 * np.sin(xx / 9.0 + rng.uniform(0, 6)) + 30 * np.cos(yy / 7.0 + rng.uniform(0, 6))
    for _ in range(6):
        y0, x0 = rng.integers(0, h - 10), rng.integers(0, w - 10)
        img[y0:y0 + rng.integers(8, 40), x0:x0 + rng.integers(8, 40)] += rng.uniform(-60, 60)
    img = img + rng.normal(0, 1.5, (h, w))
    return np.clip(np.rint(np.stack([img, img * 0.9 + 10, img * 1.05 - 5])), 0, 255)


# ---- 1. closed forms and independent formulations ---------------------------------------------------------------------------------
def test_window_is_the_stated_gaussian():
    g = NO.window()
    assert len(g) == 7 and g == g[::-1] and abs(sum(g) - 1.0) < 1e-15
    assert abs(g[3] / g[2] - math.exp(1 / (2 * (7 / 6) ** 2))) < 1e-15                        # sigma = 7/6
    assert list(NQ.NIQE_WINDOW) == g                                                          # the product's copy (niqe.hip holds the same)
    assert list(NQ.DOWN2_WEIGHTS) == NO.DOWN_W == list(RO.weights(2, False))


def test_separable_filter_against_a_direct_2d_correlation():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 255, (23, 31))
    g = np.array(NO.window())
    want = signal.correlate2d(np.pad(a, 3, mode="edge"), np.outer(g, g), mode="valid")
    assert np.max(np.abs(NO.filt(a) - want)) <= 1e-12
    assert np.array_equal(NQ._filter(a), NO.filt(a))


def test_constant_image_has_a_zero_map_and_no_usable_block():
    """Black is zero exactly; another constant c is zero up to the rounding of the window's sum (mu = c (1 +- 2^-52)), a map
    without values on both sides of zero either way: every block is dropped."""
    for value, bound in ((0.0, 0.0), (77.0, 1e-12), (255.0, 1e-12)):
        img = np.full((3, 32, 48), value)
        st, m1, m2 = NO.stats(img, 0, 16)
        assert np.max(np.abs(m1)) <= bound and np.max(np.abs(m2)) <= bound
        assert np.all(np.minimum(st[:, :, 1:25:5], st[:, :, 3:25:5]) == 0) and np.all(st[:, :, 25] <= 256 * 1e-5)   # (sigma <= c 2^-26 a pixel)
        assert not np.isfinite(NO.features(st, 16)[0]).any()
        with pytest.raises(ValueError):
            NO.niqe(img, C.MODEL_MU, C.MODEL_COV, 0, 16)
        with pytest.raises(ValueError, match="finite features"):
            NQ.niqe(img, NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, 16))


def test_scale_two_is_the_unrounded_x2_down_of_section_4f():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (24, 38)).astype(np.float64)
    want = RO.imresize(y[:, :, None], 2, up=False, rounded=False)[:, :, 0]
    assert np.array_equal(NO.down2(y), want) and np.array_equal(NQ.down2(y), want)
    t = torch.nn.functional.interpolate(torch.from_numpy(y)[None, None], scale_factor=0.5, mode="bicubic", antialias=True)[0, 0].numpy()
    assert np.max(np.abs(t[2:-2, 2:-2] - want[2:-2, 2:-2])) <= 1e-9


def test_circshift_wraps_inside_the_block():
    """4 x 4 blocks with one non-zero pair each: the pair meets through the wrap, and never through the neighbouring block."""
    # (position of 2, position of -3, index of the shifted map in which they meet)
    for p, q, which in (((0, 0), (0, 3), 1), ((0, 1), (3, 1), 2), ((0, 0), (3, 3), 3), ((0, 3), (3, 0), 4)):
        m = np.zeros((4, 8))
        m[p], m[q] = 2.0, -3.0
        m[0, 4] = 5.0                   # the first column of the second block: its left neighbour in the image is m[0, 3]
        m[3, 4] = 7.0
        for stats in (NO.block_stats(m, np.zeros_like(m), 4), NQ._block_stats(m, np.zeros_like(m), 4)):
            first = stats[0].reshape(-1)[:25].reshape(5, 5)
            for k in range(1, 5):
                assert first[k].tolist() == ([36.0, 1.0, 0.0, 0.0, 6.0] if k == which else [0.0] * 5), (p, q, k)
            assert first[0].tolist() == [9.0, 1.0, 4.0, 1.0, 5.0]
            second = stats[1].reshape(-1)[:25].reshape(5, 5)
            assert second[0].tolist() == [0.0, 0.0, 74.0, 2.0, 12.0]
            assert second[1].tolist() == [0.0] * 5 and second[3].tolist() == [0.0] * 5 and second[4].tolist() == [0.0] * 5
            assert second[2].tolist() == [0.0, 0.0, 1225.0, 1.0, 35.0]                        # 5 and 7 meet through the wrap of rows 0 and 3


# ---- 2. AGGD ----------------------------------------------------------------------------------------------------------------------
def _generalised_gaussian(shape, n, seed):
    rng = np.random.default_rng(seed)
    g = rng.gamma(1.0 / shape, 1.0, n)
    return rng.choice([-1.0, 1.0], n) * g ** (1.0 / shape)


@pytest.mark.parametrize("shape,tol", [(2.0, 0.03), (1.0, 0.015)])
def test_aggd_recovers_a_known_shape(shape, tol):
    """200 k samples, seed 1.  The restatement recovers 1.981 for shape 2 and 1.006 for shape 1 (other seeds: 1.980 .. 1.999 and
    0.997 .. 1.006): the tolerances are those errors with a margin for the sampling error of another numpy's stream."""
    x = _generalised_gaussian(shape, 200000, 1)
    five = NO.five(x)
    i, alpha, bl, br, rn, gap = NO.aggd(*five, 200000.0)
    print(f"shape {shape}: alpha {alpha}, bl {bl!r}, br {br!r}")
    assert abs(alpha - shape) <= tol
    assert abs(bl - 1.0) <= 0.02 and abs(br - 1.0) <= 0.02                                     # scale 1 on both sides
    idx, a, l, r, mean = NQ.aggd_fit([five], 200000.0)
    assert idx[0] == i and a[0] == alpha and abs(l[0] - bl) <= 1e-12 and abs(r[0] - br) <= 1e-12


def test_alpha_is_the_first_minimiser_on_a_tie():
    """ls = rs makes rn = rhat = A^2 (n = 1, L2 + R2 = 1): an A whose square is exactly midway between two neighbouring r(a) ties."""
    a, r = NO.grid()
    ties = []
    for i in range(9800):
        mid = (r[i] + r[i + 1]) / 2
        A = math.sqrt(mid)
        if (mid - r[i]) == (r[i + 1] - mid) and r[i + 1] > r[i] and A * A == mid:
            ties.append((i, A))
    assert len(ties) >= 10
    for i, A in ties[:3] + ties[-3:]:
        d = r - A * A
        assert (d * d)[i] == (d * d)[i + 1] == np.min(d * d)                                  # a tie indeed
        assert NO.aggd(0.5, 1.0, 0.5, 1.0, A, 1.0)[0] == i
        assert NQ.aggd_fit([[0.5, 1.0, 0.5, 1.0, A]], 1.0)[0][0] == i


# ---- 3. the product's host half against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,B,shave,n", [C.SHAPES[0], C.SHAPES[2], C.SHAPES[4]])
@pytest.mark.parametrize("kind,luma", [("u8", "gray"), ("float", "y")])
def test_numpy_route_and_features_against_the_restatement(h, w, B, shave, n, kind, luma):
    a, res = C.case(h, w, B, shave, n, kind, luma)
    for i, r in enumerate(res):
        st, m1, m2 = NQ.stats_numpy(a[i], shave, B, luma, return_maps=True)
        assert np.array_equal(m1, r["m1"]) and np.array_equal(m2, r["m2"])
        for sc in range(2):
            npix = (B >> sc) * (B >> sc)
            want = r["stats"][sc]
            assert np.all(np.abs(st[sc] - want) <= (npix - 1) * 2.0 ** -53 * np.abs(want))
        # fed the ORACLE's stats: the same grid indices, the rest within 1e-12 relative
        feat, index = NQ.features_from_stats(r["stats"], B, return_index=True)
        assert np.array_equal(index, r["index"])
        ok = np.isfinite(r["feat"])
        assert np.array_equal(np.isfinite(feat), ok)
        assert np.all(np.abs(feat[ok] - r["feat"][ok]) <= 1e-12 * np.abs(r["feat"][ok]))
        if r["score"] is not None:
            got = NQ.score(feat, NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, B, luma))
            assert abs(got - r["score"]) <= 1e-12 * r["score"]
    with pytest.raises(ValueError):
        NQ.features_from_stats(np.zeros((3, 4, 25)), B)


def test_model_files(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    x = rng.normal(size=(80, 36))
    m = NQ.NiqeModel(x.mean(axis=0), np.cov(x, rowvar=False), 24, "y", 80)
    m.save(tmp_path / "m.npz")
    assert sorted(os.listdir(tmp_path)) == ["m.npz"]
    k = NQ.NiqeModel.load(tmp_path / "m.npz")
    assert k.mu.tobytes() == m.mu.tobytes() and k.cov.tobytes() == m.cov.tobytes()            # bit-equal
    assert (k.block, k.luma, k.rows) == (24, "y", 80)
    with pytest.raises(ValueError, match="no such file"):
        NQ.NiqeModel.load(tmp_path / "none.npz")
    (tmp_path / "junk.npz").write_bytes(b"not a model")
    with pytest.raises(ValueError, match="not a NIQE model"):
        NQ.NiqeModel.load(tmp_path / "junk.npz")
    np.savez(tmp_path / "odd.npz", mu=m.mu, cov=m.cov, block=np.int64(25), luma=np.array("y"), rows=np.int64(1))
    with pytest.raises(ValueError, match="even"):
        NQ.NiqeModel.load(tmp_path / "odd.npz")
    # the standard model's format
    sio = pytest.importorskip("scipy.io")
    sio.savemat(tmp_path / "std.mat", {"mu_prisparam": m.mu[None, :], "cov_prisparam": m.cov})
    k = NQ.NiqeModel.load(tmp_path / "std.mat")
    assert np.array_equal(k.mu, m.mu) and np.array_equal(k.cov, m.cov) and (k.block, k.luma) == (96, "gray")
    monkeypatch.setitem(sys.modules, "scipy", None)                                           # as if scipy were not installed
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    with pytest.raises(ValueError, match="scipy"):
        NQ.NiqeModel.load(tmp_path / "std.mat")


def test_fitting_scores_and_ordering(tmp_path):
    """A model fitted from six smooth images with edges (B = 24).  Measured: smooth-plus-edge 8.57, the same with added noise 64.5,
    uniform noise 331."""
    fitset = [_smooth_edge(s) for s in range(100, 106)]
    model = NQ.fit_model(fitset, 24, "gray")
    mu, cov, rows = NO.fit_model(fitset, 24, "gray")
    assert model.rows == rows and rows >= 2 and (model.block, model.luma) == (24, "gray")
    assert np.max(np.abs(model.mu - mu)) <= 1e-12 and np.max(np.abs(model.cov - cov)) <= 1e-12
    # an image whose features have the model's mean scores 0
    feat = NQ.features_from_stats(NQ.stats_numpy(fitset[0], 0, 24), 24)
    own = NQ.NiqeModel(feat.mean(axis=0), np.cov(feat, rowvar=False), 24)
    assert NQ.score(feat, own) == 0.0 and NO.score(feat, own.mu, own.cov) <= 1e-12
    clean = _smooth_edge(7)
    rng = np.random.default_rng(8)
    noisy = np.clip(np.rint(clean + rng.normal(0, 12, clean.shape)), 0, 255)
    uniform = np.rint(rng.uniform(0, 255, clean.shape))
    got = [NQ.niqe(im, model)[0] for im in (clean, noisy, uniform)]
    print("NIQE of clean / noisy / uniform noise:", got)
    assert 0 < got[0] < got[1] < got[2]
    for im, g in zip((clean, noisy, uniform), got):
        assert abs(g - NO.niqe(im, mu, cov, 0, 24, "gray")) <= 1e-9 * g
    # utils.compute_NIQE: the numpy route for arrays and CPU tensors, a model or its path
    U = _load("utils")
    model.save(tmp_path / "m.npz")
    assert U.compute_NIQE(noisy, model) == got[1] == U.compute_NIQE(torch.from_numpy(noisy)[None].float(), str(tmp_path / "m.npz"))
    assert U.compute_NIQE(noisy, model, shave=3) == NQ.niqe(noisy[:, 3:-3, 3:-3], model)[0]
    with pytest.raises(ValueError, match="at least 2"):
        U.compute_NIQE(noisy[:, :30, :40], model)
    # the fitting CLI
    from PIL import Image
    (tmp_path / "hr").mkdir()
    for k, im in enumerate(fitset):
        Image.fromarray(im.transpose(1, 2, 0).astype(np.uint8)).save(tmp_path / "hr" / f"{k}.png")
    NQ.main(["fit", "--hr_dir", str(tmp_path / "hr"), "--out", str(tmp_path / "cli.npz"), "--block", "24"])
    cli = NQ.NiqeModel.load(tmp_path / "cli.npz")                        # (with a GPU the sums come from the kernel, in another order)
    assert cli.rows == rows and np.allclose(cli.mu, model.mu, rtol=1e-9, atol=1e-12) and np.allclose(cli.cov, model.cov, rtol=1e-9, atol=1e-12)
    with pytest.raises(SystemExit, match="--block"):
        NQ.main(["fit", "--hr_dir", str(tmp_path / "hr"), "--out", str(tmp_path / "x.npz"), "--block", "25"])
    with pytest.raises(SystemExit, match="--hr_dir"):
        NQ.main(["fit", "--hr_dir", str(tmp_path / "nowhere"), "--out", str(tmp_path / "x.npz")])


def test_golden():
    """tests/golden/gv16_niqe.npz (tests/golden/make_golden_niqe.py): a later edit of the restatement cannot move the definition
    unnoticed, and the product's numpy route lands on it."""
    assert os.path.getsize(GOLDEN) < 100 * 1024
    g = np.load(GOLDEN)
    n = int(g["count"])
    assert n == 3
    for k in range(n):
        img, (shave, B, luma) = g[f"in{k}"], g[f"par{k}"]
        mode = "y" if luma else "gray"
        st, _, _ = NO.stats(img, int(shave), int(B), mode)
        feat, index, _ = NO.features(st, int(B))
        assert np.array_equal(st, g[f"stats{k}"]) and np.array_equal(index, g[f"index{k}"])
        assert np.allclose(feat, g[f"feat{k}"], rtol=1e-13, atol=0, equal_nan=True)
        assert abs(NO.score(feat, C.MODEL_MU, C.MODEL_COV) - float(g[f"score{k}"])) <= 1e-12 * float(g[f"score{k}"])
        got = NQ.niqe(img, NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, int(B), mode), int(shave))[0]
        assert abs(got - float(g[f"score{k}"])) <= 1e-11 * float(g[f"score{k}"])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_anything_is_launched():
    """pesr_niqe_stats checks its arguments on the host first: PESR_EINVAL / PESR_EWORKSPACE come back without a device (the
    pointers are never followed on the host)."""
    from pesr_amd import _lib
    lib = _lib.lib()
    p = 0x10000
    big = 1 << 40
    call = lambda N, H, W, shave, B, luma, ws=p, nb=big: lib.pesr_niqe_stats(p, N, H, W, 0, shave, B, luma, p, None, None, ws, nb, None)
    assert call(1, 192, 192, 0, 95, 0) == -1 and call(1, 192, 192, 0, 6, 0) == -1 and call(1, 192, 192, 0, 98, 0) == -1
    assert call(1, 192, 192, -1, 96, 0) == -1
    assert call(1, 96, 191, 0, 96, 0) == -1 and call(1, 104, 199, 4, 96, 0) == -1             # one block
    assert call(1, 95, 400, 0, 96, 0) == -1                                                   # none
    assert call(0, 192, 192, 0, 96, 0) == -1 and call(65536, 192, 192, 0, 96, 0) == -1
    assert call(1, 192, 192, 0, 96, 2) == -1 and call(1, 192, 192, 0, 96, -1) == -1
    assert lib.pesr_niqe_stats(None, 1, 192, 192, 0, 0, 96, 0, p, None, None, p, big, None) == -1
    assert call(1, 96, 192, 0, 96, 0, nb=30 * 96 * 192 - 1) == -2                             # the header's formula, one byte short
    assert call(2, 200, 200, 4, 96, 1, nb=30 * 2 * 192 * 192 - 1) == -2
    assert call(1, 96, 192, 0, 96, 0, ws=None, nb=0) == -2


def test_flags_default_off_and_refusals(tmp_path, monkeypatch):
    Te, Tr = _load("test"), _load("train")
    assert Te.build_parser().parse_args([]).niqe == "" and Tr.build_parser().parse_args([]).valid_niqe == ""
    NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, 16).save(tmp_path / "m.npz")
    (tmp_path / "junk.npz").write_bytes(b"junk")
    (tmp_path / "std.mat").write_bytes(b"whatever")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match=r"test\.py: --niqe .*no such file"):
        Te.main(["--niqe", str(tmp_path / "none.npz")])
    with pytest.raises(SystemExit, match=r"test\.py: --niqe .*not a NIQE model"):
        Te.main(["--niqe", str(tmp_path / "junk.npz")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe .*no such file"):
        Tr.main(["--valid_niqe", str(tmp_path / "none.npz")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe .*not a NIQE model"):
        Tr.main(["--valid_niqe", str(tmp_path / "junk.npz")])
    # a model whose block does not fit the image twice: a 4 x 7 LR image is 16 x 28 after x4, one block of 16
    from PIL import Image
    lr = tmp_path / "data" / "origin" / "test" / "Toy" / "LR"
    lr.mkdir(parents=True)
    Image.fromarray(np.zeros((4, 7, 3), np.uint8)).save(lr / "a.png")
    with pytest.raises(SystemExit, match=r"test\.py: --niqe / --shave: a\.png: .*at least 2"):
        Te.main(["--dataset", "Toy", "--niqe", str(tmp_path / "m.npz")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe / --valid_shave / --patch_size: .*at least 2"):
        Tr.main(["--synthetic", "16", "--patch_size", "4", "--valid_niqe", str(tmp_path / "m.npz")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe / --valid_shave / --patch_size: .*at least 2"):
        Tr.main(["--synthetic", "16", "--patch_size", "8", "--valid_shave", "1", "--valid_niqe", str(tmp_path / "m.npz")])
    # a .mat without scipy
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    with pytest.raises(SystemExit, match=r"test\.py: --niqe .*scipy"):
        Te.main(["--niqe", str(tmp_path / "std.mat")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe .*scipy"):
        Tr.main(["--valid_niqe", str(tmp_path / "std.mat")])
