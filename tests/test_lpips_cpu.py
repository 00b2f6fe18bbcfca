"""CPU: LPIPS (docs/modes.md section 4n) - the ordered restatement of the head kernel (tests/lpips_oracle.py head_ordered: what the
device must equal bit for bit) against the exactly summed definition within a bound derived from the counts of rounded operations
(head_bound's docstring); the measurement behind the whole-metric tolerance of tests/test_lpips_gpu.py; the weight files
(`python -m pesr_amd.lpips pack`, LpipsModel.load); and the refusals of the C ABI, the Python layer, test.py and train.py."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import lpips_cases as C
import lpips_oracle as LO
from pesr_amd import lpips as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_lpips_" + name, os.path.join(ROOT, name + ".py"))
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


# ---- 1. the head: kernel order against the definition ------------------------------------------------------------------------------
def test_lane_shares_cover_every_channel_once():
    for c in C.CHANNELS:
        idx = LO.lane_channels(c)
        assert idx.shape == (64, c // 64) and sorted(idx.reshape(-1).tolist()) == list(range(c))
        assert idx[63, -1] == c - 1                                  # the "wone" case's channel is the last lane's last


@pytest.mark.parametrize("c,n,h,w", C.HEAD_CASES)
def test_head_ordered_within_the_derived_bound_of_head_exact(c, n, h, w):
    """|head_ordered - head_exact| <= head_bound for the map and the score of every head case: the bound is derived in
    head_bound's docstring from the number of correctly rounded operations of each d(p) (K - 1 + 6 additions per sum, one square
    root, one addition of 1e-10, one division, one subtraction, one square, one product per channel) and of the mean; every sum is
    of non-negative terms.  The GPU test then compares the device with head_ordered bit for bit and needs no tolerance."""
    for kind in C.KINDS:
        fa, fb, wt = C.head_case(c, n, h, w, kind)
        r = C.head_answers(c, n, h, w, kind)
        (so, mo), (se, me), (sb, mb) = r["ordered"], r["exact"], r["bound"]
        assert mo.shape == me.shape == (n, h, w) and so.shape == se.shape == (n,)
        assert np.isfinite(mo).all() and np.isfinite(so).all() and (mo >= 0).all()
        dm, ds = np.abs(mo - me), np.abs(so - se)
        used = float(np.max(dm / np.where(mb > 0, mb, 1.0)))
        print(f"C {c} {n} x {h} x {w} {kind}: score {se[0]!r}, largest |map difference| / bound {used:.3f}, score difference {ds.max():.3e}, "
              f"bound {sb.max():.3e}")
        assert bool((dm <= mb).all()) and bool((ds <= sb).all())
        if kind == "same":                                           # (iii)
            assert bool((mo == 0).all()) and bool((so == 0).all()) and bool((me == 0).all())
        if kind == "zeros":                                          # (ii): a pixel with both vectors zero contributes exactly 0
            both = (np.abs(fa).sum(-1) == 0) & (np.abs(fb).sum(-1) == 0)
            assert both.any() and bool((mo[both] == 0).all())
            if n * h * w >= 3:
                one = (np.abs(fa).sum(-1) == 0) ^ (np.abs(fb).sum(-1) == 0)
                assert one.any() and bool((mo[one] > 0).all())
        if kind == "near":                                           # (iv): the five-sum expansion is outside the bound, the two-pass form inside
            five = LO.head_five_sums(fa, fb, wt)
            assert bool((np.abs(five - me) > mb).any())
        if kind == "wone":                                           # (v)
            t = fa[..., c - 1].astype(np.float64) / (np.sqrt((fa.astype(np.float64) ** 2).sum(-1)) + 1e-10) \
                - fb[..., c - 1].astype(np.float64) / (np.sqrt((fb.astype(np.float64) ** 2).sum(-1)) + 1e-10)
            assert np.allclose(mo, 0.75 * t * t, rtol=1e-12, atol=0)


# ---- 2. the whole metric: how much float32 convs move it ---------------------------------------------------------------------------
def test_float32_trunk_against_float64():
    """The measurement behind tests/lpips_cases.py SCORE_RTOL: the metric with the trunk in float32 (direct convs) against the float64
    restatement.  Measured here: at most 1.218e-07 relative, at (1, 3, 16, 16) shave 0.  Every restated score is above 1e-3, so a
    relative tolerance means something."""
    worst = 0.0
    for shape, shave in C.METRIC_CASES:
        f, g = C.metric_f64(shape, shave), C.metric_trunk32(shape, shave)
        assert f.shape == (shape[0],) and bool((f > C.MIN_SCORE).all()), (shape, shave, f)
        rel = float(np.max(np.abs(f - g) / f))
        print(f"{shape} shave {shave}: lpips_f64 {f.tolist()}, float32 trunk relative difference {rel:.3e}")
        worst = max(worst, rel)
    print(f"largest {worst:.3e}; recorded {C.TRUNK32_REL:.3e}; GPU tolerance {C.SCORE_RTOL:.3e}")
    assert worst <= C.SCORE_RTOL                                     # (another BLAS may round differently: the recorded value is not re-asserted)


def test_restated_metric_properties():
    a, b = C.image_pair((1, 3, 16, 16))
    t = C.model_tensors()
    assert LO.lpips_f64(a, a, t)[0] == 0.0
    assert LO.lpips_f64(a, b, t)[0] == LO.lpips_f64(b, a, t)[0] > 0
    # the head of lpips_f64 is the head of head_exact
    with torch.no_grad():
        f = LO.trunk(torch.from_numpy(np.concatenate([a, b])), t, torch.float32)[0].permute(0, 2, 3, 1).contiguous().numpy()
    want = LO.head_exact(f[:1], f[1:], t["lin0"].numpy())[0][0]
    fa, fb = torch.from_numpy(f[:1]).double(), torch.from_numpy(f[1:]).double()
    got = (t["lin0"].double() * (fa / (fa.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
                                 - fb / (fb.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)).pow(2)).sum(-1).mean()
    assert abs(float(got) - want) <= 1e-12 * want


# ---- 3. models and files -----------------------------------------------------------------------------------------------------------
def test_random_model_is_seeded_warns_and_leaves_the_rng_alone():
    torch.manual_seed(123)
    before = torch.get_rng_state()
    with pytest.warns(UserWarning, match="no pretrained"):
        m1 = LP.LpipsModel.random(9)
    assert torch.equal(before, torch.get_rng_state())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2, m3 = LP.LpipsModel.random(9), LP.LpipsModel.random(10)
    t1, t2, t3 = m1.tensors(), m2.tensors(), m3.tensors()
    assert all(torch.equal(t1[k], t2[k]) for k in t1 if k != "format") and not torch.equal(t1["conv0.weight"], t3["conv0.weight"])
    assert len(m1.convs) == 13 and [tuple(c.weight.shape[:2]) for c in m1.convs] == LP.conv_shapes()
    assert [w.numel() for w in m1.lins] == [64, 128, 256, 512, 512] and all(bool((w >= 0).all()) for w in m1.lins)
    assert not any(p.requires_grad for p in m1.parameters())
    # the input affine is img / 127.5 - 1, then (x - shift) / scale
    x = torch.tensor([0.0, 100.0, 255.0])
    for ch in range(3):
        want = ((x.double() / 127.5 - 1) - LP.SHIFT[ch]) / LP.SCALE[ch]
        got = x.double() * m1.scaling.weight[ch, ch, 0, 0].double() + m1.scaling.bias[ch].double()
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
    assert float(m1.scaling.weight.abs().sum()) == pytest.approx(sum(1 / (127.5 * s) for s in LP.SCALE), rel=1e-6)


def _published_pair(seed=0):
    """Synthetic stand-ins for the two published files: a torchvision-style vgg16 state_dict and the LPIPS v0.1 linear layers."""
    g = torch.Generator().manual_seed(seed)
    vgg = {}
    for idx, (cout, cin) in zip(LP.TORCHVISION_CONVS, LP.conv_shapes()):
        vgg[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
        vgg[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
    vgg["classifier.0.weight"] = torch.zeros(4, 4)                  # what the trunk does not use is ignored
    lin = {k: torch.rand(1, c, 1, 1, generator=g) for k, c in zip(LP.LIN_KEYS, LP.TAP_CHANNELS)}
    return vgg, lin


def test_pack_round_trip_and_refusals(tmp_path):
    assert LP.TORCHVISION_CONVS == (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    assert LP.LIN_KEYS == tuple(f"lin{l}.model.1.weight" for l in range(5))
    vgg, lin = _published_pair()
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    LP.main(["pack", "--vgg16", str(tmp_path / "vgg16.pth"), "--lin", str(tmp_path / "lin.pth"), "--out", str(tmp_path / "lpips_vgg.pt")])
    m = LP.LpipsModel.load(str(tmp_path / "lpips_vgg.pt"))
    for i, idx in enumerate(LP.TORCHVISION_CONVS):
        assert torch.equal(m.convs[i].weight, vgg[f"features.{idx}.weight"]) and torch.equal(m.convs[i].bias, vgg[f"features.{idx}.bias"])
    for l, k in enumerate(LP.LIN_KEYS):
        assert torch.equal(m.lins[l], lin[k].reshape(-1))
    m.save(tmp_path / "again.pt")
    t1, t2 = m.tensors(), LP.LpipsModel.load(str(tmp_path / "again.pt")).tensors()
    assert t1.keys() == t2.keys() and all(torch.equal(t1[k], t2[k]) for k in t1 if k != "format")
    # a wrong shape and a missing key each exit naming the key
    bad = dict(vgg)
    bad["features.10.weight"] = torch.zeros(256, 128, 3, 2)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(SystemExit, match=r"--vgg16 .*features\.10\.weight has shape"):
        LP.main(["pack", "--vgg16", str(tmp_path / "bad.pth"), "--lin", str(tmp_path / "lin.pth"), "--out", str(tmp_path / "x.pt")])
    bad = dict(vgg)
    del bad["features.28.bias"]
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(SystemExit, match=r"--vgg16 .*features\.28\.bias is missing"):
        LP.main(["pack", "--vgg16", str(tmp_path / "bad.pth"), "--lin", str(tmp_path / "lin.pth"), "--out", str(tmp_path / "x.pt")])
    bad = dict(lin)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    torch.save(bad, tmp_path / "badlin.pth")
    with pytest.raises(SystemExit, match=r"--lin .*lin3\.model\.1\.weight has shape"):
        LP.main(["pack", "--vgg16", str(tmp_path / "vgg16.pth"), "--lin", str(tmp_path / "badlin.pth"), "--out", str(tmp_path / "x.pt")])
    bad = dict(lin)
    del bad["lin0.model.1.weight"]
    torch.save(bad, tmp_path / "badlin.pth")
    with pytest.raises(SystemExit, match=r"--lin .*lin0\.model\.1\.weight is missing"):
        LP.main(["pack", "--vgg16", str(tmp_path / "vgg16.pth"), "--lin", str(tmp_path / "badlin.pth"), "--out", str(tmp_path / "x.pt")])
    bad = dict(lin)
    bad["lin2.model.1.weight"] = -bad["lin2.model.1.weight"] - 1
    torch.save(bad, tmp_path / "badlin.pth")
    with pytest.raises(SystemExit, match=r"lin2: negative"):
        LP.main(["pack", "--vgg16", str(tmp_path / "vgg16.pth"), "--lin", str(tmp_path / "badlin.pth"), "--out", str(tmp_path / "x.pt")])
    with pytest.raises(SystemExit, match=r"--vgg16 .*no such file"):
        LP.main(["pack", "--vgg16", str(tmp_path / "none.pth"), "--lin", str(tmp_path / "lin.pth"), "--out", str(tmp_path / "x.pt")])
    assert not (tmp_path / "x.pt").exists()
    # load's own refusals
    with pytest.raises(ValueError, match="no such file"):
        LP.LpipsModel.load(str(tmp_path / "none.pt"))
    (tmp_path / "junk.pt").write_bytes(b"junk")
    with pytest.raises(ValueError, match="not readable"):
        LP.LpipsModel.load(str(tmp_path / "junk.pt"))
    with pytest.raises(ValueError, match="not an LPIPS weight file"):
        LP.LpipsModel.load(str(tmp_path / "vgg16.pth"))
    d = m.tensors()
    del d["conv4.bias"]
    torch.save(d, tmp_path / "short.pt")
    with pytest.raises(ValueError, match=r"conv4\.bias: missing"):
        LP.LpipsModel.load(str(tmp_path / "short.pt"))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_anything_is_launched():
    """pesr_lpips_layer checks its arguments on the host first: PESR_EINVAL / PESR_EWORKSPACE come back without a device (the
    pointers are never followed on the host)."""
    from pesr_amd import _lib
    lib = _lib.lib()
    assert "pesr_lpips_layer" in _lib.SIGNATURES
    p, big = 0x10000, 1 << 40
    call = lambda N, H, W, Cc, feat=p, ws=p, nb=big: lib.pesr_lpips_layer(feat, p, p, N, H, W, Cc, None, ws, nb, None)
    for c in (96, 0, 32, 63, 192, 1024, -64):
        assert call(1, 8, 8, c) == -1, c
    assert call(0, 8, 8, 64) == -1 and call(65536, 8, 8, 64) == -1 and call(1, 0, 8, 64) == -1 and call(1, 8, 0, 64) == -1
    assert call(1, 8, 8, 64, feat=None) == -1 and call(1, 8, 8, 64, feat=p + 4) == -1
    assert call(2, 9, 7, 64, nb=8 * 2 * 1 - 1) == -2 and call(2, 67, 129, 64, nb=8 * 2 * 136 - 1) == -2      # the header's formula, one byte short
    assert call(1, 8, 8, 64, ws=None, nb=0) == -2


def test_python_layer_has_no_cpu_path(gpu_untouched):
    U = _load("utils")
    m = C.model()
    a = torch.zeros(1, 3, 32, 32)
    with pytest.raises(ValueError, match="no CPU path"):
        LP.lpips(a, a, m)
    with pytest.raises(ValueError, match="no CPU path"):
        U.compute_LPIPS(a, a, m)
    with pytest.raises(ValueError, match="no CPU path"):
        U.compute_LPIPS(a.numpy(), a.numpy(), m)
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError):
        ops.lpips_layer(torch.zeros(2, 4, 4, 64), torch.zeros(64))
    assert not gpu_untouched


def test_flags_default_off_and_refusals(tmp_path, monkeypatch, gpu_untouched):
    Te, Tr = _load("test"), _load("train")
    assert Te.build_parser().parse_args([]).lpips == "" and Tr.build_parser().parse_args([]).valid_lpips == ""
    C.model().save(tmp_path / "w.pt")
    (tmp_path / "junk.pt").write_bytes(b"junk")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match=r"test\.py: --lpips .*--from_hr true"):
        Te.main(["--lpips", str(tmp_path / "w.pt")])
    with pytest.raises(SystemExit, match=r"test\.py: --lpips .*--from_hr true"):
        Te.main(["--lpips", "x"])
    with pytest.raises(SystemExit, match=r"test\.py: --lpips .*no such file"):
        Te.main(["--from_hr", "true", "--lpips", str(tmp_path / "none.pt")])
    with pytest.raises(SystemExit, match=r"test\.py: --lpips .*not readable"):
        Te.main(["--from_hr", "true", "--lpips", str(tmp_path / "junk.pt")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_lpips .*no such file"):
        Tr.main(["--valid_lpips", str(tmp_path / "none.pt")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_lpips .*not readable"):
        Tr.main(["--valid_lpips", str(tmp_path / "junk.pt")])
    # images that the four pools would leave nothing of: 20 x 40 HR, 12 x 32 after --shave 4
    from PIL import Image
    hr = tmp_path / "data" / "origin" / "test" / "Toy" / "HR"
    hr.mkdir(parents=True)
    Image.fromarray(np.zeros((20, 40, 3), np.uint8)).save(hr / "a.png")
    with pytest.raises(SystemExit, match=r"test\.py: --lpips / --shave: a\.png: 12 x 32 .*16 x 16"):
        Te.main(["--dataset", "Toy", "--from_hr", "true", "--shave", "4", "--lpips", str(tmp_path / "w.pt")])
    with pytest.raises(SystemExit, match=r"train\.py: --valid_lpips / --valid_shave / --patch_size: .*12 x 12 .*16 x 16"):
        Tr.main(["--synthetic", "16", "--patch_size", "4", "--valid_shave", "2", "--valid_lpips", str(tmp_path / "w.pt")])
    assert not gpu_untouched
