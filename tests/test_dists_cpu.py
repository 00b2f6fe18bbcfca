"""CPU: DISTS (docs/modes.md section 4t) - the float64 definition (tests/dists_oracle.py dists_f64) against a literal transcription of
the published forward; the ordered restatement of the head kernels (layer_ordered: what the device must equal bit for bit) against
exactly summed statistics, within a derived bound (stats_bound's docstring); the measurement behind the whole-metric tolerance of
tests/test_dists_gpu.py; the weight files (`python -m pesr_amd.dists pack`, DistsModel.load); the Scorer's column; and the refusals of
the C ABI, the Python layer, test.py and train.py."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import dists_cases as C
import dists_oracle as DO
import lpips_cases as LC
from pesr_amd import dists as DS
from pesr_amd import lpips as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_dists_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture
def gpu_untouched(monkeypatch):
    """Every initialisation of torch.cuda from here on is recorded (and refused); the test asserts that there was none."""
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise AssertionError("torch.cuda was initialised")
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    return calls


# ---- 1. the definition -------------------------------------------------------------------------------------------------------------
def test_definition_against_the_published_forward():
    """dists_f64 (the centred two-pass statistics, one sum per stage) equals the literal transcription of the published forward
    (xy_cov = mean(x y) - mean_x mean_y, dist1 and dist2 apart) to 1e-12 absolute on every case: the centred form is the same quantity."""
    t = C.model_tensors()
    for shape, shave in C.TRUNK32_CASES:
        a, b = C.image_pair(shape, shave)
        f = C.metric_f64(shape, shave)[0] if (shape, shave) in C.METRIC_CASES else DO.dists_f64(a, b, t, shave)
        p = DO.dists_published(a, b, t, shave)
        print(f"{shape} shave {shave}: dists_f64 {f.tolist()}, published form {p.tolist()}, difference {np.max(np.abs(f - p)):.3e}")
        assert f.shape == p.shape == (shape[0],) and np.isfinite(f).all()
        assert float(np.max(np.abs(f - p))) <= 1e-12
        assert bool((f > 1e-4).all()) and bool((f < 1).all())          # a pair that differs scores above zero


def test_identical_and_constant_images():
    t = C.model_tensors()
    a, b = C.image_pair((2, 3, 17, 23))
    same = DO.dists_f64(a, a, t)
    print(f"identical images: {same.tolist()}")
    assert float(np.max(np.abs(same))) <= 1475 * 2.0 ** -53           # S1 = S2 = 1 on every channel; the weights sum to one within rounding
    assert np.array_equal(DO.dists_f64(a, b, t), DO.dists_f64(b, a, t))
    # two constant images with different constants: zero variance and covariance in stage 0, S2 = c2 / c2 = 1 there
    ca, cb = np.full((1, 3, 16, 16), 40.0, np.float32), np.full((1, 3, 16, 16), 200.0, np.float32)
    score = DO.dists_f64(ca, cb, t)
    assert np.isfinite(score).all() and 0 < float(score[0]) < 1
    x = np.concatenate([ca, cb]).transpose(0, 2, 3, 1) / np.float32(255)
    ones = np.ones(3)
    _, stats = DO.layer_ordered(x[:1], x[1:], ones, ones)
    assert bool((stats[0, :, 2:] == 0).all())                         # var_a = var_b = cov = 0 exactly
    only_s2, _ = DO.layer_ordered(x[:1], x[1:], 0 * ones, ones)
    assert only_s2[0] == 3.0                                          # beta = 1 on three channels: S2 = 1 on each


# ---- 2. the head: kernel order against exactly summed statistics -------------------------------------------------------------------
@pytest.mark.parametrize("c,hw", [(c, hw) for c, hw in C.LAYER_CASES if c <= 64])
def test_layer_ordered_within_the_derived_bound_of_exact_statistics(c, hw):
    """|layer_ordered's statistics - stats_exact| <= stats_bound, of order P * 2^-53 relative to each statistic's own scale, for every
    kind; at mean 1e3 and spread 1e-2 the uncentred one-pass form is outside that bound and the centred form inside.  (C = 512 runs
    the same per-channel arithmetic: the exact rational sums are taken at C = 3 and 64 only, for time.)"""
    for kind in C.KINDS:
        fa, fb, alpha, beta = C.layer_case(c, hw, kind)
        contrib, got = C.layer_ordered(c, hw, kind)
        ex, bound = DO.stats_exact(fa, fb), DO.stats_bound(fa, fb)
        assert got.shape == ex.shape == (C.LAYER_N, c, 5) and contrib.shape == (C.LAYER_N,) and np.isfinite(got).all()
        d = np.abs(got - ex)
        used = float(np.max(d / np.where(bound > 0, bound, 1.0)))
        print(f"C {c} {hw} {kind}: largest |difference| / bound {used:.3f}; var_a {ex[0, 0, 2]!r}, bound {bound[0, 0, 2]:.3e}")
        assert bool((d <= bound).all())
        P = hw[0] * hw[1]
        if kind == "mean" and P > 1:
            scale = np.stack([np.abs(ex[..., 0]), np.abs(ex[..., 1]), ex[..., 2], ex[..., 3], np.sqrt(ex[..., 2] * ex[..., 3])], axis=-1)
            assert bool((bound <= 200 * 2.0 ** -53 * np.maximum(scale, 1e-300) * max(P, 64)).all())      # the bound IS of that order
            un = DO.stats_uncentred(fa, fb)
            assert bool((np.abs(un[..., 2:] - ex[..., 2:]) > bound[..., 2:]).any())
        if kind == "zero":                                           # a channel of zeros in both maps: S1 = S2 = 1
            assert bool((got[:, c - 1] == 0).all())
            one = np.zeros(c)
            one[c - 1] = 1.0
            assert bool((DO.layer_ordered(fa, fb, one, one)[0] == 2.0).all())
        # the contribution is the weighted sum of S1 and S2 of those statistics
        s1 = (2 * ex[..., 0] * ex[..., 1] + 1e-6) / (ex[..., 0] ** 2 + ex[..., 1] ** 2 + 1e-6)
        s2 = (2 * ex[..., 4] + 1e-6) / (ex[..., 2] + ex[..., 3] + 1e-6)
        if kind != "mean":                                           # (at mean 1e3 S2's own sensitivity to var ~ 1e-4 is what the bound is for)
            assert np.allclose(contrib, (alpha * s1 + beta * s2).sum(-1), rtol=1e-10, atol=0)


def test_l2pool_restatement():
    """l2pool_f64 is the published L2pooling: hanning(5)[1:-1] outer itself, normalised; stride 2, padding 1; ceil(H/2) x ceil(W/2)."""
    a = np.hanning(5)[1:-1]
    g = a[:, None] * a[None, :]
    g = g / g.sum()
    assert np.array_equal(g, np.outer([1, 2, 1], [1, 2, 1]) / 16.0)
    for n, h, w, c in C.L2POOL_CASES:
        x, y = C.l2pool_case(n, h, w, c)
        assert y.shape == (n, -(-h // 2), -(-w // 2), c) and y.dtype == np.float64
        xx = np.zeros((n, h + 2, w + 2, c))
        xx[:, 1:h + 1, 1:w + 1] = x.astype(np.float64) ** 2
        oy, ox = y.shape[1] - 1, y.shape[2] - 1                       # the last window, which reaches the padding on an odd side
        want = np.sqrt((xx[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3] * g[None, :, :, None]).sum(axis=(1, 2)) + 1e-12)
        assert np.allclose(y[:, oy, ox], want, rtol=1e-14, atol=0)
    assert np.array_equal(DO.l2pool_f64(np.zeros((1, 3, 3, 64), np.float32)), np.full((1, 2, 2, 64), np.sqrt(1e-12)))


# ---- 3. the whole metric: how much a float32 trunk moves it ------------------------------------------------------------------------
def test_float32_trunk_against_float64():
    """The measurement behind tests/dists_cases.py SCORE_ATOL: the metric with the trunk in float32 (direct convs, fp32 pooling)
    against the float64 definition, as tests/test_lpips_cpu.py::test_float32_trunk_against_float64 does for LPIPS - but absolute,
    because the score is one minus a sum near one.  The measurement must not exceed the recorded value."""
    worst, where = 0.0, None
    for shape, shave in C.TRUNK32_CASES:
        a, b = C.image_pair(shape, shave)
        f = C.metric_f64(shape, shave)[0] if (shape, shave) in C.METRIC_CASES else DO.dists_f64(a, b, C.model_tensors(), shave)
        g = C.metric_trunk32(shape, shave)
        diff = float(np.max(np.abs(f - g)))
        print(f"{shape} shave {shave}: dists_f64 {f.tolist()}, float32 trunk absolute difference {diff:.3e}, relative {np.max(np.abs(f - g) / f):.3e}")
        if diff > worst:
            worst, where = diff, (shape, shave)
    print(f"largest {worst:.3e} at {where}; recorded {C.TRUNK32_ABS:.3e}; GPU tolerance {C.SCORE_ATOL:.3e}")
    assert 0 < worst <= C.TRUNK32_ABS


# ---- 4. models and files -----------------------------------------------------------------------------------------------------------
def test_random_model_is_seeded_warns_and_leaves_the_rng_alone():
    torch.manual_seed(123)
    before = torch.get_rng_state()
    with pytest.warns(UserWarning, match="no pretrained"):
        m1 = DS.DistsModel.random(9)
    assert torch.equal(before, torch.get_rng_state())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2, m3 = DS.DistsModel.random(9), DS.DistsModel.random(10)
    t1, t2, t3 = m1.tensors(), m2.tensors(), m3.tensors()
    assert all(torch.equal(t1[k], t2[k]) for k in t1 if k != "format") and not torch.equal(t1["alpha"], t3["alpha"])
    assert len(m1.convs) == 13 and [tuple(c.weight.shape[:2]) for c in m1.convs] == LP.conv_shapes()
    assert m1.alpha.shape == m1.beta.shape == (1475,) and m1.alpha.dtype == m1.beta.dtype == torch.float64
    assert DS.STAGE_CHANNELS == (3, 64, 128, 256, 512, 512) and DS.CHANNELS == 1475
    assert abs(float(m1.alpha.mean()) - 0.1) < 2e-3 and 5e-3 < float(m1.alpha.std()) < 2e-2
    assert not any(p.requires_grad for p in m1.parameters())
    aw, bw = m1.normalised(torch.device("cpu"))
    assert aw.dtype == torch.float64 and abs(float(aw.sum() + bw.sum()) - 1.0) <= 1475 * 2.0 ** -53
    assert m1.weight_sum() == DO.weight_sum(t1)
    # the two input affines: img / 255, and (img / 255 - mean) / std
    x = torch.tensor([0.0, 100.0, 255.0])
    for ch in range(3):
        want = (x.double() / 255 - DS.MEAN[ch]) / DS.STD[ch]
        got = x.double() * m1.scaling.weight[ch, ch, 0, 0].double() + m1.scaling.bias[ch].double()
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
        assert float(m1.unit.weight[ch, ch, 0, 0]) == float(np.float32(1) / np.float32(255)) and float(m1.unit.bias[ch]) == 0.0
    assert float(m1.unit.weight.abs().sum()) == pytest.approx(3 / 255, rel=1e-6)


def _published_pair(seed=0):
    """Synthetic stand-ins for the two published files: a torchvision-style vgg16 state_dict and the DISTS weights.pt."""
    g = torch.Generator().manual_seed(seed)
    vgg = {}
    for idx, (cout, cin) in zip(LP.TORCHVISION_CONVS, LP.conv_shapes()):
        vgg[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
        vgg[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
    vgg["classifier.0.weight"] = torch.zeros(4, 4)                  # what the trunk does not use is ignored
    w = {"alpha": 0.1 + 0.01 * torch.randn(1, 1475, 1, 1, generator=g), "beta": 0.1 + 0.01 * torch.randn(1, 1475, 1, 1, generator=g)}
    return vgg, w


def test_pack_round_trip_and_refusals(tmp_path):
    vgg, w = _published_pair()
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(w, tmp_path / "weights.pt")
    args = lambda v="vgg16.pth", ww="weights.pt": ["pack", "--vgg16", str(tmp_path / v), "--weights", str(tmp_path / ww), "--out", str(tmp_path / "x.pt")]
    DS.main(["pack", "--vgg16", str(tmp_path / "vgg16.pth"), "--weights", str(tmp_path / "weights.pt"), "--out", str(tmp_path / "dists_vgg.pt")])
    m = DS.DistsModel.load(str(tmp_path / "dists_vgg.pt"))
    for i, idx in enumerate(LP.TORCHVISION_CONVS):
        assert torch.equal(m.convs[i].weight, vgg[f"features.{idx}.weight"]) and torch.equal(m.convs[i].bias, vgg[f"features.{idx}.bias"])
    assert torch.equal(m.alpha, w["alpha"].reshape(-1).double()) and torch.equal(m.beta, w["beta"].reshape(-1).double())
    m.save(tmp_path / "again.pt")
    t1, t2 = m.tensors(), DS.DistsModel.load(str(tmp_path / "again.pt")).tensors()
    assert t1["format"] == DS.FORMAT == "pesr_amd.dists vgg16 v1"
    assert t1.keys() == t2.keys() and all(torch.equal(t1[k], t2[k]) for k in t1 if k != "format")
    # flat alpha / beta pack to the same model
    torch.save({k: v.reshape(-1) for k, v in w.items()}, tmp_path / "flat.pt")
    assert torch.equal(DS.pack(vgg, torch.load(tmp_path / "flat.pt")).alpha, m.alpha)

    def refused(match, vgg_sd=None, w_sd=None):
        torch.save(vgg if vgg_sd is None else vgg_sd, tmp_path / "v.pth")
        torch.save(w if w_sd is None else w_sd, tmp_path / "w.pt")
        with pytest.raises(SystemExit, match=match):
            DS.main(args("v.pth", "w.pt"))
    bad = dict(vgg)
    bad["features.10.weight"] = torch.zeros(256, 128, 3, 2)
    refused(r"--vgg16 .*features\.10\.weight has shape", vgg_sd=bad)
    bad = dict(vgg)
    del bad["features.28.bias"]
    refused(r"--vgg16 .*features\.28\.bias is missing", vgg_sd=bad)
    bad = dict(vgg)
    bad["features.0.bias"] = torch.full((64,), float("nan"))
    refused(r"conv0\.bias: non-finite", vgg_sd=bad)
    refused(r"--weights .*key beta is missing", w_sd={"alpha": w["alpha"]})
    refused(r"--weights .*key alpha has shape \(1, 1474, 1, 1\)", w_sd={"alpha": w["alpha"][:, :1474], "beta": w["beta"]})
    bad = {"alpha": w["alpha"].clone(), "beta": w["beta"]}
    bad["alpha"][0, 7] = float("inf")
    refused(r"alpha: non-finite", w_sd=bad)
    refused(r"sum\(alpha\) \+ sum\(beta\) = .* is not positive", w_sd={"alpha": -w["alpha"], "beta": -w["beta"]})
    refused(r"sum\(alpha\) \+ sum\(beta\) = 0\.0 is not positive", w_sd={"alpha": 0 * w["alpha"], "beta": 0 * w["beta"]})
    with pytest.raises(SystemExit, match=r"dists pack: --vgg16 .*no such file"):
        DS.main(args("none.pth"))
    assert not (tmp_path / "x.pt").exists()
    # load's own refusals
    with pytest.raises(ValueError, match="no such file"):
        DS.DistsModel.load(str(tmp_path / "none.pt"))
    (tmp_path / "junk.pt").write_bytes(b"junk")
    with pytest.raises(ValueError, match="not readable"):
        DS.DistsModel.load(str(tmp_path / "junk.pt"))
    with pytest.raises(ValueError, match="not a DISTS weight file"):
        DS.DistsModel.load(str(tmp_path / "vgg16.pth"))              # a file that is no model
    LC.model().save(tmp_path / "lpips.pt")
    with pytest.raises(ValueError, match="an LPIPS weight file"):
        DS.DistsModel.load(str(tmp_path / "lpips.pt"))
    with pytest.raises(ValueError, match="not an LPIPS weight file"):
        LP.LpipsModel.load(str(tmp_path / "dists_vgg.pt"))            # and the other way round
    d = m.tensors()
    del d["conv4.bias"]
    torch.save(d, tmp_path / "short.pt")
    with pytest.raises(ValueError, match=r"conv4\.bias: missing"):
        DS.DistsModel.load(str(tmp_path / "short.pt"))
    d = m.tensors()
    d["beta"] = d["beta"][:100]
    with pytest.raises(ValueError, match=r"beta: shape \(100,\), expected \(1475,\)"):
        DS.DistsModel.from_tensors(d, "x")
    d = m.tensors()
    d["alpha"][3] = float("nan")
    with pytest.raises(ValueError, match=r"alpha: non-finite"):
        DS.DistsModel.from_tensors(d, "x")
    with pytest.raises(SystemExit, match=r"test\.py: --dists .*no such file"):
        DS.load_model_flag("test.py", "--dists", str(tmp_path / "none.pt"))


# ---- 5. the Scorer -----------------------------------------------------------------------------------------------------------------
def test_scorer_columns_and_refusals(tmp_path, gpu_untouched):
    from pesr_amd.quality import Scorer
    dm, lm = C.model(), LC.model()
    dm.save(tmp_path / "d.pt")
    assert Scorer("test.py", True, 0, "", lm, dists=dm).columns() == ["PSNR-Y", "SSIM-Y", "LPIPS", "DISTS"]
    assert Scorer("test.py", False, 0, dists=dm).columns() == ["PSNR-Y", "DISTS"]
    assert Scorer("test.py", False, 0, dists=str(tmp_path / "d.pt")).dists_model is not None
    assert Scorer("test.py", True, 0, "", lm).columns() == ["PSNR-Y", "SSIM-Y", "LPIPS"]          # without DISTS: what it was
    assert Scorer("test.py", False, 0).dists_model is None
    assert Scorer("test.py", False, 0, dists=dm).columns(hr=False) == []
    import niqe_cases as NC
    from pesr_amd.niqe import NiqeModel
    full = Scorer("test.py", True, 2, NiqeModel(NC.MODEL_MU, NC.MODEL_COV, 16), lm, dists=dm)
    assert full.columns() == ["PSNR-Y", "SSIM-Y", "NIQE", "LPIPS", "DISTS"] and full.columns(hr=False) == ["NIQE"]
    a = {"PSNR-Y": 30.5, "LPIPS": 0.125, "DISTS": 0.0625}
    b = {"PSNR-Y": 28.25, "LPIPS": 0.25, "DISTS": 0.5}
    assert Scorer.test_line(a, b) == ("PSNR-Y 30.5000000000 dB, bicubic 28.2500000000 dB, LPIPS 0.1250000000, bicubic 0.2500000000, "
                                      "DISTS 0.0625000000, bicubic 0.5000000000")
    assert list(Scorer.valid_lines(1, 1, {"PSNR-Y": 30.5, "DISTS": 0.0625})) == [
        ("Finish valid [1/1]. PSNR: 30.5000dB", "Validate PSNR", 30.5), ("Finish valid [1/1]. DISTS: 0.062500", "Validate DISTS", 0.0625)]
    with pytest.raises(SystemExit, match=r"test\.py: --dists compares the result with the HR image: it needs --from_hr true"):
        Scorer("test.py", False, 0, have_hr=False, dists=dm)
    with pytest.raises(SystemExit, match=r"train\.py: --valid_dists .*no such file"):
        Scorer("train.py", False, 0, dists=str(tmp_path / "none.pt"), dists_flag="--valid_dists")
    s = Scorer("test.py", False, 4, dists=dm)
    s.check_size(24, 40, "ok.png")
    with pytest.raises(SystemExit, match=r"test\.py: --dists / --shave: a\.png: 12 x 32 after the shave; DISTS needs at least 16 x 16"):
        s.check_size(20, 40, "a.png")
    t = Scorer("train.py", False, 2, flags=("--valid_niqe", "--valid_lpips", "--valid_shave"), size_flags="--valid_shave / --patch_size",
               dists=dm, dists_flag="--valid_dists")
    with pytest.raises(SystemExit, match=r"train\.py: --valid_dists / --valid_shave / --patch_size: the synthetic validation images: 12 x 12 "
                                         r"after the shave; DISTS needs at least 16 x 16"):
        t.check_size(16, 16, "the synthetic validation images")
    # a score that cannot be taken names the DISTS flag: here a CPU tensor
    from pesr_amd.quality import ScoreError
    only = Scorer("test.py", False, 0, dists=dm)
    only.columns = lambda hr=True: ["DISTS"]
    with pytest.raises(ScoreError, match="no CPU path") as e:
        only.score(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))
    assert e.value.flags == "--dists / --shave"
    assert not gpu_untouched


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_host_side_refusals():
    """The new symbols are in the header and in _lib.SIGNATURES, the library exports them, and the version is 19; the launchers check
    their arguments on the host first (the pointers are never followed there)."""
    import re
    from pesr_amd import _lib
    names = ("pesr_l2pool_blocks", "pesr_l2pool_fwd", "pesr_dists_pixel_blocks", "pesr_dists_workspace_bytes", "pesr_dists_layer")
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    for name in names:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pesr_abi_version() == 20
    p, big = 0x10000, 1 << 40
    pool = lambda N, H, W, Cc, x=p, y=p: lib.pesr_l2pool_fwd(x, y, N, H, W, Cc, None)
    for c in (0, 3, 32, 96, -64):
        assert pool(1, 8, 8, c) == -1 and lib.pesr_l2pool_blocks(1, 8, 8, c) == 0, c
    assert pool(0, 8, 8, 64) == -1 and pool(1, 0, 8, 64) == -1 and pool(1, 8, 0, 64) == -1
    assert pool(1, 8, 8, 64, x=None) == -1 and pool(1, 8, 8, 64, y=None) == -1 and pool(1, 8, 8, 64, x=p + 4) == -1
    assert lib.pesr_l2pool_blocks(2, 5, 7, 64) == -(-2 * 3 * 4 * 16 // 256) and lib.pesr_l2pool_blocks(1, 1, 1, 64) == 1
    layer = lambda N, H, W, Cc, feat=p, ws=p, nb=big: lib.pesr_dists_layer(feat, p, p, p, N, H, W, Cc, None, ws, nb, None)
    for c in (0, 1, 4, 32, 96, 192, 1024, -64):
        assert layer(1, 8, 8, c) == -1 and lib.pesr_dists_pixel_blocks(1, 64, c) == 0 and lib.pesr_dists_workspace_bytes(1, 64, c) == 0, c
    assert layer(0, 8, 8, 64) == -1 and layer(32768, 8, 8, 64) == -1 and layer(1, 0, 8, 64) == -1 and layer(1, 8, 0, 64) == -1
    assert layer(1, 8, 8, 64, feat=None) == -1 and layer(1, 8, 8, 64, feat=p + 2) == -1
    assert [lib.pesr_dists_pixel_blocks(2, P, 64) for P in (1, 256, 257, 573)] == [1, 1, 2, 3] == \
        [-(-P // DO.BLOCK_PIX) for P in (1, 256, 257, 573)]
    need = lib.pesr_dists_workspace_bytes(2, 573, 512)
    assert need == 8 * 2 * 512 * 5 * (3 + 1)                          # the five partial sums per block, and their five results
    assert layer(2, 3, 191, 512, nb=need - 1) == -2 and layer(2, 3, 191, 512, ws=None, nb=0) == -2


def test_python_layer_has_no_cpu_path(gpu_untouched):
    U = _load("utils")
    m = C.model()
    a = torch.zeros(1, 3, 32, 32)
    with pytest.raises(ValueError, match="no CPU path"):
        DS.dists(a, a, m)
    with pytest.raises(ValueError, match="no CPU path"):
        U.compute_DISTS(a, a, m)
    with pytest.raises(ValueError, match="no CPU path"):
        U.compute_DISTS(a.numpy(), a.numpy(), m)
    from pesr_amd import _lib, ops
    one = torch.ones(64, dtype=torch.float64)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat"):
        ops.dists_layer(torch.zeros(2, 4, 4, 64), one, one)
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x"):
        ops.l2pool_fwd(torch.zeros(2, 4, 4, 64))
    assert ops.dists_plan(2, 257, 64)["pixel_blocks"] == 2 and ops.dists_plan(2, 256, 3)["pixel_blocks"] == 1
    assert ops.dists_plan(2, 257, 64)["pixels_per_block"] == DO.BLOCK_PIX
    with pytest.raises(ValueError, match="dists_plan"):
        ops.dists_plan(2, 64, 96)
    assert not gpu_untouched


def test_flags_default_off_and_refusals(tmp_path, monkeypatch, gpu_untouched):
    Te, Tr = _load("test"), _load("train")
    assert Te.build_parser().parse_args([]).dists == "" and Tr.build_parser().parse_args([]).valid_dists == ""
    C.model().save(tmp_path / "w.pt")
    LC.model().save(tmp_path / "lpips.pt")
    (tmp_path / "junk.pt").write_bytes(b"junk")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match=r"test\.py: --dists .*--from_hr true"):
        Te.main(["--dists", str(tmp_path / "w.pt")])
    with pytest.raises(SystemExit, match=r"test\.py: --dists .*no such file"):
        Te.main(["--from_hr", "true", "--dists", str(tmp_path / "none.pt")])
    with pytest.raises(SystemExit, match=r"test\.py: --dists .*not readable"):
        Te.main(["--from_hr", "true", "--dists", str(tmp_path / "junk.pt")])
    with pytest.raises(SystemExit, match=r"test\.py: --dists .*an LPIPS weight file"):
        Te.main(["--from_hr", "true", "--dists", str(tmp_path / "lpips.pt")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_dists .*no such file"):
        Tr.main(["--valid_dists", str(tmp_path / "none.pt")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_dists .*not readable"):
        Tr.main(["--valid_dists", str(tmp_path / "junk.pt")])
    # an image that the shave leaves too little of: 20 x 40 HR, 12 x 32 after --shave 4
    from PIL import Image
    hr = tmp_path / "data" / "origin" / "test" / "Toy" / "HR"
    hr.mkdir(parents=True)
    Image.fromarray(np.zeros((20, 40, 3), np.uint8)).save(hr / "a.png")
    with pytest.raises(SystemExit, match=r"test\.py: --dists / --shave: .*a\.png: 12 x 32 after the shave; DISTS needs at least 16 x 16"):
        Te.main(["--dataset", "Toy", "--from_hr", "true", "--dists", str(tmp_path / "w.pt"), "--shave", "4"])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_dists / --valid_shave / --patch_size: the synthetic validation images: 12 x 12 "
                                         r"after the shave; DISTS needs at least 16 x 16"):
        Tr.main(["--synthetic", "16", "--patch_size", "4", "--valid_dists", str(tmp_path / "w.pt"), "--valid_shave", "2"])
    assert not gpu_untouched
