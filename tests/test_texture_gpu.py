"""GPU: the texture loss (docs/modes.md section 4q).

The Gram kernels of pesr_amd/csrc/gram.hip against float64 of the same fp32 inputs (tests/texture_oracle.py) within first-order
bounds that are derived, not measured: K (forward) or C (backward) products and additions with one rounding each.  Symmetry,
reproducibility and the separation of images bit for bit; the distance kernel against an exact sum of the device's own Gram matrices;
the autograd node end to end; the VGG taps; the GAN step with the term off, on and captured.  Shapes are the smallest at which each
path runs: one and several patches, an odd K (the k tail), every channel count, one and several staged pieces, split-K."""
import math

import numpy as np
import pytest
import torch

import texture_oracle as O
import loss_step_harness as HS
from oracle import detrand

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 2


def _smallest_split_shape():
    """The smallest whole-map shape with C = 64 that the launcher cuts along K (smallest area, then smallest height)."""
    from pesr_amd import ops
    for area, h in sorted((h * w, h) for h in range(1, 65) for w in range(1, 65)):
        if ops.gram_plan(N, h, area // h, 64, h, area // h)["splits"] > 1:
            return h, area // h
    raise AssertionError("no whole-map shape up to 64 x 64 is split")


# (C, H, W, patch): several patches; an odd K; one patch of one staged piece (C = 128: 64 pixels) ... and of four; C = 256 with two
# patches of eight pieces; the smallest split shape (appended below) and a split one with an odd K and an uneven last slice.  TAILS
# (behind the split shape, so that every earlier case keeps its index and its seeds): K = 35 at C = 256 (a backward run of 32 and a
# tail of 3; the forward's tile groups at an odd K) and at C = 128 (one backward run with a tail of 35)
CASES = [(64, 8, 8, 4), (64, 5, 7, 0), (128, 16, 16, 16), (256, 16, 32, 16), (64, 23, 23, 0)]
TAILS = [(256, 5, 7, 0), (128, 5, 7, 0)]
_SHARED = {}


def _cases():
    if "cases" not in _SHARED:
        h, w = _smallest_split_shape()
        _SHARED["cases"] = CASES + [(64, h, w, 0)] + TAILS
    return _SHARED["cases"]


def _case(i):
    """Inputs, device results and float64 references of case i, computed once."""
    key = ("case", i)
    if key not in _SHARED:
        from pesr_amd import ops
        c, h, w, patch = _cases()[i]
        fa, fb = O.features(10 + i, N, h, w, c), O.features(40 + i, N, h, w, c)
        assert fa.min() < 0 < fa.max() and abs(float(fa.mean())) > 0.1
        g = np.array([0.75, -1.5])
        da, db = torch.from_numpy(fa).to(DEV), torch.from_numpy(fb).to(DEV)
        Ga, Gb = ops.gram(da, patch), ops.gram(db, patch)
        t, dg = ops.gram_loss(Ga, Gb, True)
        gf = ops.gram_bwd(da, dg, torch.from_numpy(g).to(DEV), patch)
        ph, pw = O.patch_of(h, w, patch)
        _SHARED[key] = dict(c=c, h=h, w=w, patch=patch, ph=ph, pw=pw, fa=fa, fb=fb, g=g, da=da, db=db, Ga=Ga, Gb=Gb, t=t, dg=dg, gf=gf,
                            plan=ops.gram_plan(N, h, w, c, ph, pw))
    return _SHARED[key]


NCASES = len(CASES) + 1 + len(TAILS)


def test_the_cases_cover_the_paths():
    cases = _cases()
    assert len(cases) == NCASES
    plans = [_case(i)["plan"] for i in range(NCASES)]
    assert [p["splits"] for p in plans[:4]] == [1, 1, 1, 1]
    assert plans[4]["splits"] > 1 and plans[4]["pixels"] % 2 == 1     # split, odd K
    assert plans[5]["splits"] > 1, plans[5]                           # the smallest shape the launcher splits
    print("smallest split shape with C = 64:", cases[5], plans[5])
    assert plans[1]["pixels"] == 35 and plans[0]["patches"] == 4 and plans[3]["patches"] == 2
    assert [(c[0], p["pixels"], p["splits"]) for c, p in zip(cases[6:], plans[6:])] == [(256, 35, 1), (128, 35, 1)]


# ---- the Gram matrices --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASES))
def test_gram_against_float64_within_the_derived_bound(i):
    """|G - G64| <= (K + 8) 2^-24 s sum_k |F_kc F_kc'| per entry: the first-order bound for K products and K additions with one rounding
    each, in any order (so split-K too), plus the scale.  Worst ratio of the error to the bound seen on the MI355X: 0.175 (docs/modes.md 4q)."""
    k = _case(i)
    for f, G in ((k["fa"], k["Ga"]), (k["fb"], k["Gb"])):
        want, bound = O.gram(f, k["patch"]), O.gram_bound(f, k["patch"])
        got = G.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape == (N, k["plan"]["patches"], k["c"], k["c"])
        ratio = float(np.max(np.abs(got.astype(np.float64) - want) / bound))
        print(f"gram {k['c']} x {k['h']} x {k['w']} patch {k['patch']} splits {k['plan']['splits']}: worst |error| / bound = {ratio:.4f}")
        assert bound.min() > 0 and ratio <= 1.0


@pytest.mark.parametrize("i", range(NCASES))
def test_gram_is_symmetric_reproducible_and_keeps_images_apart(i):
    from pesr_amd import ops
    k = _case(i)
    G = k["Ga"]
    assert torch.equal(G, G.transpose(2, 3))                          # bit for bit
    assert torch.equal(ops.gram(k["da"], k["patch"]), G)              # the same call, the same bits
    other = k["da"].clone()
    other[0] = k["db"][0]
    G2 = ops.gram(other, k["patch"])
    assert torch.equal(G2[1], G[1]) and torch.equal(G2[0], k["Gb"][0]) and not torch.equal(G2[0], G[0])


# ---- the distance --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASES))
def test_distance_and_difference(i):
    from pesr_amd import ops
    k = _case(i)
    a64, b64 = k["Ga"].cpu().numpy().astype(np.float64), k["Gb"].cpu().numpy().astype(np.float64)
    d = a64 - b64                                                     # exact: both are float32
    P, count = d.shape[1], d[0].size
    t = k["t"].cpu().numpy()
    assert k["t"].dtype == torch.float64 and t.shape == (N,)
    for n in range(N):
        want = math.fsum((d[n].ravel() ** 2).tolist()) / P
        err = abs(t[n] - want) / want
        print(f"t[{n}] = {t[n]!r}: {err:.3e} relative to the exact sum, allowed {count * 2.0 ** -53:.3e}")
        assert want > 0 and err <= count * 2.0 ** -53
    dg = k["dg"].cpu().numpy()
    assert dg.dtype == np.float32 and np.array_equal(dg, d.astype(np.float32))     # one rounding of the exact difference
    assert np.array_equal(dg, dg.transpose(0, 1, 3, 2))
    t2, none = ops.gram_loss(k["Ga"], k["Gb"], False)
    assert none is None and torch.equal(t2, k["t"])
    t0, dg0 = ops.gram_loss(k["Ga"], k["Ga"], True)
    assert t0.tolist() == [0.0] * N and not bool(dg0.any())           # equal inputs: exactly 0


# ---- the gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASES))
def test_backward_against_float64_within_the_derived_bound(i):
    """Against float64 of the same F, the device's own fp32 dG and g: (C + 8) 2^-24 |g| (4 s / P) sum_c' |dG F| per element."""
    from pesr_amd import ops
    k = _case(i)
    dg = k["dg"].cpu().numpy()
    want, bound = O.grad_from_dg(k["fa"], dg, k["g"], k["patch"]), O.grad_bound(k["fa"], dg, k["g"], k["patch"])
    got = k["gf"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == k["fa"].shape
    ratio = float(np.max(np.abs(got.astype(np.float64) - want) / bound))
    print(f"gram_bwd {k['c']} x {k['h']} x {k['w']} patch {k['patch']}: worst |error| / bound = {ratio:.4f}")
    assert bound.min() > 0 and ratio <= 1.0
    assert torch.equal(ops.gram_bwd(k["da"], k["dg"], torch.from_numpy(k["g"]).to(DEV), k["patch"]), k["gf"])
    zero = ops.gram_bwd(k["da"], k["dg"], torch.tensor([k["g"][0], 0.0], dtype=torch.float64, device=DEV), k["patch"])
    assert torch.equal(zero[0], k["gf"][0]) and not bool(zero[1].any())


# ---- the autograd node end to end ------------------------------------------------------------------------------------------------------
# Against the float64 oracle on the fp32 features.  These two cannot be derived tightly (dG cancels), so they are measured: on these
# eight cases on the MI355X the worst relative error of T was 5.03e-8 (64 x 23 x 23, whole map) and the worst error of the gradient
# 6.51e-7 of the largest gradient entry (256 x 16 x 32, patch 16); the other cases: T 3.1e-9 .. 4.5e-8, gradient 2.5e-7 .. 4.7e-7
# (docs/modes.md section 4q).  Four times the measured value is allowed, to leave room for other seeds.
T_MEASURED, GRAD_MEASURED = 5.03e-8, 6.51e-7
T_ALLOWED, GRAD_ALLOWED = 4 * T_MEASURED, 4 * GRAD_MEASURED


@pytest.mark.parametrize("i", range(NCASES))
def test_texture_layer_end_to_end(i):
    from pesr_amd import functional as PF
    k = _case(i)
    fa = k["da"].clone().requires_grad_(True)
    fb = k["db"].clone().requires_grad_(True)
    t = PF.texture_layer(fa, fb, k["patch"])
    assert t.dtype == torch.float64 and t.shape == (N,) and torch.equal(t.detach(), k["t"])
    (t * torch.from_numpy(k["g"]).to(DEV)).sum().backward()
    assert fb.grad is None and torch.equal(fa.grad, k["gf"])
    want_t, want_g = O.layer(k["fa"], k["fb"], k["patch"]), O.layer_grad(k["fa"], k["fb"], k["g"], k["patch"])
    e_t = float(np.max(np.abs(t.detach().cpu().numpy() - want_t) / want_t))
    e_g = float(np.max(np.abs(fa.grad.cpu().numpy().astype(np.float64) - want_g))) / float(np.max(np.abs(want_g)))
    print(f"texture_layer {k['c']} x {k['h']} x {k['w']} patch {k['patch']}: T {e_t:.3e} relative (allowed {T_ALLOWED:.1e}), "
          f"gradient {e_g:.3e} of the largest entry (allowed {GRAD_ALLOWED:.1e})")
    assert e_t <= T_ALLOWED and e_g <= GRAD_ALLOWED
    plain = PF.texture_layer(k["da"], k["db"], k["patch"])            # nothing needs a gradient: the pure value
    assert not plain.requires_grad and torch.equal(plain, k["t"])


def test_ops_refuse_what_they_do_not_take():
    from pesr_amd import _lib, ops
    f = torch.zeros(N, 8, 8, 64, device=DEV)
    with pytest.raises(_lib.PesrHipError, match="does not tile"):
        ops.gram(f, 3)
    with pytest.raises(_lib.PesrHipError, match="C = 96"):
        ops.gram(torch.zeros(N, 8, 8, 96, device=DEV), 0)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.gram(f.permute(0, 2, 1, 3)[:, :, ::2], 0)                 # a view
    G = ops.gram(f, 4)
    with pytest.raises(_lib.PesrHipError, match="differ in shape"):
        ops.gram_loss(G, G[:, :2].contiguous())
    with pytest.raises(_lib.PesrHipError, match="dg"):
        ops.gram_bwd(f, G[:, :2].contiguous(), torch.ones(N, dtype=torch.float64, device=DEV), 4)
    with pytest.raises(_lib.PesrHipError, match="float64"):
        ops.gram_bwd(f, G, torch.ones(N, device=DEV), 4)


# ---- the VGG taps -----------------------------------------------------------------------------------------------------------------------
_vgg = HS.vgg


@pytest.mark.parametrize("path", ["merged", "plain"])
@pytest.mark.parametrize("h,w", [(16, 16), (32, 48)])
def test_vgg_taps_leave_the_features_and_their_gradient_alone(h, w, path):
    from pesr_amd import functional as PF
    from pesr_amd import texture
    from pesr_amd.model.basic import nhwc
    V = _vgg()
    sr0, hr = detrand.image_batch((N, 3, h, w), 300).cuda(), detrand.image_batch((N, 3, h, w), 301).cuda()
    last = list(V.vgg.parameters())[-1]
    last.requires_grad = path == "plain"                              # a trainable tail takes the per-pass path
    try:
        out = []
        for taps in (False, True):
            sr = sr0.clone().requires_grad_(True)
            res = V(sr, hr, taps=taps)
            assert len(res) == (4 if taps else 2)
            PF.mse_loss(nhwc(res[0]), nhwc(res[1])).backward()        # the taps requested but unused
            out.append((res, sr.grad))
    finally:
        last.requires_grad = False
        last.grad = None
    (a0, b0), g0 = out[0]
    (a1, b1, taps_sr, taps_hr), g1 = out[1]
    assert torch.equal(a1, a0) and torch.equal(b1, b0)                # bit for bit
    assert float(g0.abs().max()) > 0 and np.array_equal(g1.cpu().numpy(), g0.cpu().numpy())      # a mask is a select
    assert len(taps_sr) == len(taps_hr) == 3
    for l, (ts, th, c) in enumerate(zip(taps_sr, taps_hr, texture.TAP_CHANNELS)):
        assert tuple(ts.shape) == tuple(th.shape) == (N, h >> l, w >> l, c)
        assert float(ts.min()) >= 0 and float(th.min()) >= 0 and float(ts.max()) > 0
        assert ts.requires_grad and not th.requires_grad
    assert texture.tap_sizes(h, w) == [tuple(t.shape[1:3]) for t in taps_sr]


@pytest.mark.parametrize("mode", ["bf16", "split-bf16"])
def test_texture_from_taps_under_the_bf16_modes(mode):
    """The convs run in their mode, the Gram kernels in fp32: the value is finite, positive and has a gradient."""
    from pesr_amd import ops, texture
    V = _vgg()
    sr = detrand.image_batch((N, 3, 32, 32), 302).cuda().requires_grad_(True)
    hr = detrand.image_batch((N, 3, 32, 32), 303).cuda()
    old = ops.PRECISION
    ops.set_precision(mode)
    try:
        _, _, taps_sr, taps_hr = V(sr, hr, taps=True)
        assert all(t.dtype == torch.float32 for t in taps_sr)
        T = texture.texture_from_taps(taps_sr, taps_hr, 8)
        T.sum().backward()
    finally:
        ops.set_precision(old)
    assert T.dtype == torch.float64 and T.shape == (N,) and bool(torch.isfinite(T).all()) and float(T.min()) > 0
    assert bool(torch.isfinite(sr.grad).all()) and float(sr.grad.abs().max()) > 0


def test_texture_from_taps_is_the_oracle_on_the_taps():
    from pesr_amd import texture
    V = _vgg()
    sr = detrand.image_batch((N, 3, 32, 32), 304).cuda()
    hr = detrand.image_batch((N, 3, 32, 32), 305).cuda()
    with torch.no_grad():
        _, _, taps_sr, taps_hr = V(sr, hr, taps=True)
    a, b = [t.cpu().numpy() for t in taps_sr], [t.cpu().numpy() for t in taps_hr]
    for patch in (8, 0):
        got = texture.texture_from_taps(taps_sr, taps_hr, patch).cpu().numpy()
        want, bound = O.texture(a, b, patch), O.texture_bound(a, b, patch)
        err = np.abs(got - want)
        print(f"texture_from_taps on the VGG taps, patch {patch}: T {float(np.max(err / want)):.3e} relative, "
              f"{float(np.max(err / bound)):.4f} of the bound derived from the Gram matrices' bounds")
        assert got.dtype == np.float64 and want.min() > 0 and bool((err <= bound).all()), (patch, got, want, bound)
    with pytest.raises(ValueError, match="3 taps"):
        texture.texture_from_taps(taps_sr[:2], taps_hr[:2], 0)


# ---- the GAN step ------------------------------------------------------------------------------------------------------------------------
# (off, on beside the other logs, and captured: tests/test_loss_terms_gpu.py, for every term, on this harness)
BATCH, ALPHA = 2, 0.5                                                 # toy networks; the HR side is 32: taps of 32, 16 and 8 pixels
H = HS.harness(350, BATCH)                                            # 64 channels, 2 blocks, LR 8 x 8, lr 5e-5


@pytest.mark.parametrize("patch", [8, 0])
def test_step_with_the_term_on(patch):
    from pesr_amd import texture
    logs4, states4, calls = H.run(4, alpha_texture=ALPHA, texture_patch=patch)
    logs0, states0, _ = H.run(2)
    assert calls == [{"taps": texture.TAPS}] * 4 and texture.TAPS == (1, 6, 11)
    got = logs4[0]["texture"]
    tr = H.trainer(alpha_texture=ALPHA, texture_patch=patch)
    lr, hr = H.data()[0]
    with torch.no_grad():                                             # the sr of the first step: G before its update
        _, _, taps_sr, taps_hr = tr.vgg(tr.G(lr), hr, taps=True)
    a, b = [t.cpu().numpy() for t in taps_sr], [t.cpu().numpy() for t in taps_hr]
    want, bound = float(O.texture(a, b, patch).mean()) * ALPHA, float(O.texture_bound(a, b, patch).mean()) * ALPHA
    print(f"patch {patch}: logged texture term {got!r}, restated {want!r}, derived bound {bound:.3e}")
    assert np.isfinite(got) and got > 0 and abs(got - want) <= bound + 2.0 ** -22 * want      # (the mean and the weight are fp32)
    HS.assert_only_G_moved(logs4[0], states4[0], logs0[0], states0[0])
