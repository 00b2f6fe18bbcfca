"""GPU: the contextual loss (docs/modes.md section 4r).

The stages of pesr_amd/csrc/cx.hip against float64 (tests/contextual_oracle.py): the normalised points, the distances and the second
GEMM within first-order bounds that are derived, not measured; the row minima bit for bit from the device's own D; the selections
equal to the oracle's (tests/test_contextual_cpu.py asserts the gaps that make this a fair demand); the exp chain end to end within four
times what was measured; reproducibility, the separation of images and the zero gradient bit for bit; the VGG's tuple taps; the GAN
step with the term off, on, beside the texture term, and captured.  Shapes are the smallest at which each path runs."""
import numpy as np
import pytest
import torch

import contextual_oracle as O
import loss_step_harness as HS
from oracle import detrand

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 2
H_BAND = 0.5
G_UP = np.array([0.75, -1.5])

# (C, H, W, regime, seed): P = 16 under one tile; P = 35 odd tails in both GEMM dimensions; exactly one row block; a block and a tail
# (the cross-block column maximum); several blocks with many-to-one arg maxima; P = 35 again at C = 128 (the tails of that channel
# count's staging and backward tiles); and, appended, the smallest P with two staged column pieces.  The seeds are those whose inputs
# tests/test_contextual_cpu.py checks.
CASES = [(64, 4, 4, "matched", 100), (64, 5, 7, "unmatched", 110), (128, 8, 8, "matched", 120), (256, 8, 9, "unmatched", 130),
         (256, 16, 16, "unmatched", 141), (128, 5, 7, "unmatched", 166)]
LAST = (64, 5, 13, "matched", 151)
NCASES = len(CASES) + 1
_SHARED = {}


def _smallest_two_piece_points():
    from pesr_amd import ops
    for p in range(1, 4097):
        if ops.cx_plan(N, p, 64)["col_pieces"] > 1:
            return p
    raise AssertionError("no P up to 4096 has two column pieces")


def _cases():
    if "cases" not in _SHARED:
        p = _smallest_two_piece_points()
        assert p == LAST[1] * LAST[2], p                              # (tests/test_contextual_cpu.py checked the inputs of this shape)
        _SHARED["cases"] = CASES + [LAST]
    return _SHARED["cases"]


def _case(i):
    """Inputs, device results and float64 references of case i, computed once."""
    key = ("case", i)
    if key not in _SHARED:
        from pesr_amd import ops
        c, h, w, regime, seed = _cases()[i]
        fa, fb = O.features(seed, N, h, w, c, regime)
        da, db = torch.from_numpy(fa).to(DEV), torch.from_numpy(fb).to(DEV)
        xh, yh, inv, mu = ops.cx_normalize(da, db)
        D, m, b = ops.cx_dist(xh, yh)
        L, CX, S, a, cmax = ops.cx_fwd(D, m, H_BAND, c)
        g = torch.from_numpy(G_UP).to(DEV)
        gf, E, gxh = ops.cx_bwd(g, xh, yh, inv, D, m, b, S, a, cmax, CX, H_BAND, (N, h, w, c), parts=True)
        _SHARED[key] = dict(c=c, h=h, w=w, P=h * w, regime=regime, fa=fa, fb=fb, da=da, db=db, xh=xh, yh=yh, inv=inv, mu=mu, D=D, m=m, b=b,
                            L=L, CX=CX, S=S, a=a, cmax=cmax, g=g, gf=gf, E=E, gxh=gxh, plan=ops.cx_plan(N, h * w, c),
                            ref=O.grad(fa, fb, G_UP, H_BAND))
    return _SHARED[key]


def _name(k):
    return f"{k['c']} x {k['h']} x {k['w']} {k['regime']}"


def test_the_cases_cover_the_paths():
    cases = _cases()
    assert len(cases) == NCASES
    plans = [_case(i)["plan"] for i in range(NCASES)]
    print("plans:", plans)
    assert [_case(i)["P"] for i in range(NCASES)] == [16, 35, 64, 72, 256, 35, 65]
    assert [p["row_blocks"] for p in plans] == [1, 1, 1, 2, 4, 1, 2]  # under a tile, odd, exactly one block, a block and a tail, several
    assert [p["col_pieces"] for p in plans] == [1, 1, 1, 2, 4, 1, 2]
    assert sorted({c[0] for c in cases}) == [64, 128, 256]
    for i, (c, h, w, regime, _) in enumerate(cases):                  # many-to-one arg maxima where the inputs are unmatched
        a = _case(i)["ref"]["a"]
        assert all((len(set(a[n].tolist())) < h * w) == (regime == "unmatched") for n in range(N))


# ---- the stages within derived bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASES))
def test_normalised_points_against_float64_within_the_derived_bound(i):
    """Against float64 of the same fp32 inputs; the bound is contextual_oracle.normalize_bound's.  Worst ratio seen on the MI355X: see
    docs/modes.md section 4r."""
    k = _case(i)
    bx, by = O.normalize_bound(k["fa"], k["fb"])
    worst = 0.0
    for got, want, bound in ((k["xh"], k["ref"]["xh"], bx), (k["yh"], k["ref"]["yh"], by)):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (N, k["P"], k["c"]) and bound.min() > 0
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want.numpy()) / bound)))
    e_inv = float(np.max(np.abs(k["inv"].cpu().numpy() / k["ref"]["inv"].numpy() - 1)))
    e_mu = float(np.max(np.abs(k["mu"].cpu().numpy() - k["ref"]["mu"].numpy()) / np.abs(k["ref"]["mu"].numpy())))
    print(f"normalize {_name(k)}: worst |error| / bound = {worst:.4f}; inv {e_inv:.2e}, mu {e_mu:.2e} relative")
    assert worst <= 1.0 and e_mu <= 1.01 * O.U32


@pytest.mark.parametrize("i", range(NCASES))
def test_distances_against_float64_within_the_derived_bound_and_row_minima_bit_for_bit(i):
    """D against float64 of the device's own xh, yh: (C + 8) 2^-24 (1/2) sum_c |xh_ic yh_jc| plus one rounding of d; m and b bit for bit
    the minimum of the device's own D and its lowest index."""
    k = _case(i)
    xh, yh = k["xh"].cpu().numpy().astype(np.float64), k["yh"].cpu().numpy().astype(np.float64)
    want = (1.0 - np.einsum("nic,njc->nij", xh, yh)) / 2.0
    bound = O.dist_bound(xh, yh)
    D = k["D"].cpu().numpy()
    assert D.dtype == np.float32 and D.shape == (N, k["P"], k["P"])
    ratio = float(np.max(np.abs(D.astype(np.float64) - want) / bound))
    print(f"dist {_name(k)}: worst |error| / bound = {ratio:.4f}")
    assert bound.min() > 0 and ratio <= 1.0
    assert np.array_equal(k["m"].cpu().numpy(), D.min(axis=2))
    assert k["b"].dtype == torch.int32 and np.array_equal(k["b"].cpu().numpy(), D.argmin(axis=2))      # numpy: the first of equal minima


@pytest.mark.parametrize("i", range(NCASES))
def test_selections_are_the_oracles(i):
    k = _case(i)
    assert np.array_equal(k["b"].cpu().numpy(), k["ref"]["b"].numpy())
    assert k["a"].dtype == torch.int32 and np.array_equal(k["a"].cpu().numpy(), k["ref"]["a"].numpy())


@pytest.mark.parametrize("i", range(NCASES))
def test_second_gemm_against_float64_within_the_derived_bound(i):
    """g_xh = -E yh / 2 against float64 of the device's own E and yh: (P + 8) 2^-24 (1/2) sum_j |E_ij yh_jc| per element.  E itself (the
    exp chain) is only measured: against float64 of the device's own D, m, b, S, a, cmax, CX."""
    k = _case(i)
    E, yh = k["E"].cpu().numpy().astype(np.float64), k["yh"].cpu().numpy().astype(np.float64)
    want, bound = -0.5 * np.einsum("nij,njc->nic", E, yh), O.gxh_bound(E, yh)
    got = k["gxh"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (N, k["P"], k["c"])
    err = np.abs(got.astype(np.float64) - want)
    zero = bound == 0                                                 # a row that no column selects has E = 0 exactly, and so g_xh = 0
    assert bool((err[zero] == 0).all()) and not zero.all()
    ratio = float(np.max(err[~zero] / bound[~zero]))
    E64 =O.e_matrix(k["D"].cpu().numpy(), k["m"].cpu().numpy(), k["b"].cpu().numpy(), k["S"].cpu().numpy(), k["a"].cpu().numpy(),
                     k["cmax"].cpu().numpy(), k["CX"].cpu().numpy(), G_UP, H_BAND).numpy()
    e_e = float(np.max(np.abs(E - E64)) / np.max(np.abs(E64)))
    print(f"g_xh {_name(k)}: worst |error| / bound = {ratio:.4f}; E {e_e:.3e} of its largest entry")
    assert ratio <= 1.0
    if k["regime"] == "matched":
        assert not zero.any()


# ---- end to end: the exp chain cannot be bounded tightly, so it is measured ----------------------------------------------------------------
# Against the float64 oracle on the same fp32 features, on these seven cases on the MI355X (docs/modes.md section 4r has every case):
# the worst |CX - CX64| / CX64 (128 x 5 x 7; the other six: 1.7e-8 .. 1.052e-7) and the worst gradient error relative to the largest
# gradient entry.  Four times the measured value is allowed, the convention of tests/test_texture_gpu.py, to leave room for other seeds.
CX_MEASURED, GRAD_MEASURED = 3.729e-7, 3.121e-6
CX_ALLOWED, GRAD_ALLOWED = 4 * CX_MEASURED, 4 * GRAD_MEASURED


@pytest.mark.parametrize("i", range(NCASES))
def test_contextual_layer_end_to_end(i):
    from pesr_amd import functional as PF
    k = _case(i)
    fa = k["da"].clone().requires_grad_(True)
    fb = k["db"].clone().requires_grad_(True)
    L = PF.contextual_layer(fa, fb, H_BAND)
    assert L.dtype == torch.float64 and L.shape == (N,) and torch.equal(L.detach(), k["L"])
    (L * k["g"]).sum().backward()
    assert fb.grad is None and torch.equal(fa.grad, k["gf"])          # fb never gets a gradient
    ref = k["ref"]
    cx64, l64 = ref["CX"].numpy(), ref["L"].numpy()
    e_cx = float(np.max(np.abs(k["CX"].cpu().numpy() - cx64) / cx64))
    e_l = float(np.max(np.abs(L.detach().cpu().numpy() - l64) / l64))
    e_g = float(np.max(np.abs(fa.grad.cpu().numpy().astype(np.float64) - ref["gf"]))) / float(np.max(np.abs(ref["gf"])))
    e_s = float(np.max(np.abs(k["S"].cpu().numpy() / ref["S"].numpy() - 1)))
    print(f"contextual_layer {_name(k)}: CX {e_cx:.3e} relative (allowed {CX_ALLOWED:.1e}), L {e_l:.3e} relative, S {e_s:.3e} relative, "
          f"gradient {e_g:.3e} of the largest entry (allowed {GRAD_ALLOWED:.1e}); L = {L.tolist()}")
    assert 0 < float(k["CX"].min()) and float(k["CX"].max()) < 1
    l_dev = k["L"].cpu().numpy()
    assert float(np.max(np.abs(l_dev + np.log(k["CX"].cpu().numpy())) / l_dev)) <= 2.0 ** -50      # L is -log of the device's CX, in double
    assert e_cx <= CX_ALLOWED and e_g <= GRAD_ALLOWED
    plain = PF.contextual_layer(k["da"], k["db"], H_BAND)             # nothing needs a gradient: the pure value
    assert not plain.requires_grad and torch.equal(plain, k["L"])


# ---- behaviour, bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(NCASES))
def test_two_calls_give_equal_bits_and_images_stay_apart(i):
    from pesr_amd import ops
    k = _case(i)

    def run(da, db, g):
        xh, yh, inv, _ = ops.cx_normalize(da, db)
        D, m, b = ops.cx_dist(xh, yh)
        L, CX, S, a, cmax = ops.cx_fwd(D, m, H_BAND, k["c"])
        return xh, yh, D, m, b, L, CX, S, a, cmax, ops.cx_bwd(g, xh, yh, inv, D, m, b, S, a, cmax, CX, H_BAND, tuple(da.shape))
    again = run(k["da"], k["db"], k["g"])
    for got, name in zip(again, ("xh", "yh", "D", "m", "b", "L", "CX", "S", "a", "cmax", "gf")):
        assert torch.equal(got, k[name]), name
    da, db = k["da"].clone(), k["db"].clone()
    da[0], db[0] = k["db"][0].flip(0), k["da"][0]                     # another image 0
    other = run(da, db, k["g"])
    for got, name in zip(other, ("xh", "yh", "D", "m", "b", "L", "CX", "S", "a", "cmax", "gf")):
        assert torch.equal(got[1], k[name][1]), name
        assert not torch.equal(got[0], k[name][0]) or name in ("a", "b"), name
    zero = run(k["da"], k["db"], torch.tensor([G_UP[0], 0.0], dtype=torch.float64, device=DEV))[-1]
    assert torch.equal(zero[0], k["gf"][0]) and not bool(zero[1].any()) and bool(k["gf"][1].any())


def test_ops_refuse_what_they_do_not_take():
    from pesr_amd import _lib, ops
    f = torch.zeros(N, 4, 4, 64, device=DEV)
    with pytest.raises(_lib.PesrHipError, match="C = 96"):
        ops.cx_normalize(torch.zeros(N, 4, 4, 96, device=DEV), torch.zeros(N, 4, 4, 96, device=DEV))
    with pytest.raises(_lib.PesrHipError, match="P = 4160"):
        ops.cx_normalize(torch.zeros(1, 65, 64, 64, device=DEV), torch.zeros(1, 65, 64, 64, device=DEV))
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.cx_normalize(f.permute(0, 2, 1, 3)[:, :, ::2], f)           # a view
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.cx_normalize(f.double(), f.double())
    with pytest.raises(_lib.PesrHipError, match="differ in shape"):
        ops.cx_normalize(f, f[:, :2].contiguous())
    xh, yh, inv, _ = ops.cx_normalize(f + 1, f)
    with pytest.raises(_lib.PesrHipError, match="cx_dist.yh"):
        ops.cx_dist(xh, yh[:, :8].contiguous())
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        ops.cx_dist(xh.transpose(1, 2), yh)
    D, m, b = ops.cx_dist(xh, yh)
    with pytest.raises(_lib.PesrHipError, match="h must be > 0"):
        ops.cx_fwd(D, m, 0.0, 64)
    with pytest.raises(_lib.PesrHipError, match="cx_fwd.m"):
        ops.cx_fwd(D, m.double(), 0.5, 64)
    L, CX, S, a, cmax = ops.cx_fwd(D, m, 0.5, 64)
    with pytest.raises(_lib.PesrHipError, match="cx_bwd.gL"):
        ops.cx_bwd(torch.ones(N, device=DEV), xh, yh, inv, D, m, b, S, a, cmax, CX, 0.5)
    with pytest.raises(_lib.PesrHipError, match="cx_bwd.a"):
        ops.cx_bwd(torch.ones(N, dtype=torch.float64, device=DEV), xh, yh, inv, D, m, b, S, a.long(), cmax, CX, 0.5)


# ---- the VGG taps -----------------------------------------------------------------------------------------------------------------------
_vgg = HS.vgg


@pytest.mark.parametrize("path", ["merged", "plain"])
@pytest.mark.parametrize("h,w", [(16, 16), (32, 48)])
def test_vgg_tuple_taps_leave_the_features_and_their_gradient_alone(h, w, path):
    from pesr_amd import contextual
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    V = _vgg()
    sr0, hr = detrand.image_batch((N, 3, h, w), 300).cuda(), detrand.image_batch((N, 3, h, w), 301).cuda()
    last = list(V.vgg.parameters())[-1]
    last.requires_grad = path == "plain"                              # a trainable tail takes the per-pass path
    try:
        out = []
        for taps in (False, True, (contextual.TAP,), (1, 6, 11, contextual.TAP)):
            sr = sr0.clone().requires_grad_(True)
            res = V(sr, hr, taps=taps)
            assert len(res) == (4 if taps else 2)
            PF.mse_loss(nhwc(res[0]), nhwc(res[1])).backward()        # the taps requested but unused
            out.append((res, sr.grad))
    finally:
        last.requires_grad = False
        last.grad = None
    (a0, b0), g0 = out[0]
    assert float(g0.abs().max()) > 0
    for res, g in out[1:]:
        assert torch.equal(res[0], a0) and torch.equal(res[1], b0)    # bit for bit
        assert np.array_equal(g.cpu().numpy(), g0.cpu().numpy())      # a mask is a select
    three, one, four = out[1][0], out[2][0], out[3][0]
    assert len(three[2]) == 3 and len(one[2]) == len(one[3]) == 1 and len(four[2]) == len(four[3]) == 4
    for l in range(3):                                                # the first three of the four are the taps of taps=True
        assert torch.equal(four[2][l], three[2][l]) and torch.equal(four[3][l], three[3][l])
    assert torch.equal(four[2][3], one[2][0]) and torch.equal(four[3][3], one[3][0])
    ts, th = one[2][0], one[3][0]
    assert tuple(ts.shape) == tuple(th.shape) == (N, h // 4, w // 4, contextual.TAP_CHANNELS) == (N,) + contextual.tap_size(h, w) + (256,)
    assert ts.is_contiguous() and th.is_contiguous() and ts.dtype == torch.float32                 # NHWC
    assert float(ts.detach().min()) >= 0 and float(th.min()) >= 0 and float(ts.detach().max()) > 0
    assert ts.requires_grad and not th.requires_grad


@pytest.mark.parametrize("mode", ["bf16", "split-bf16"])
def test_contextual_from_tap_under_the_bf16_modes(mode):
    """The convs run in their mode, the contextual kernels in fp32: the value is finite, positive and has a gradient."""
    from pesr_amd import contextual, ops
    V = _vgg()
    sr = detrand.image_batch((N, 3, 32, 32), 302).cuda().requires_grad_(True)
    hr = detrand.image_batch((N, 3, 32, 32), 303).cuda()
    old = ops.PRECISION
    ops.set_precision(mode)
    try:
        _, _, taps_sr, taps_hr = V(sr, hr, taps=(contextual.TAP,))
        assert taps_sr[0].dtype == torch.float32
        L = contextual.contextual_from_tap(taps_sr[0], taps_hr[0], H_BAND)
        L.sum().backward()
    finally:
        ops.set_precision(old)
    assert L.dtype == torch.float64 and L.shape == (N,) and bool(torch.isfinite(L).all()) and float(L.min()) > 0
    assert bool(torch.isfinite(sr.grad).all()) and float(sr.grad.abs().max()) > 0


# ---- the GAN step ------------------------------------------------------------------------------------------------------------------------
# (off, on beside the other logs, and captured: tests/test_loss_terms_gpu.py, for every term, on this harness)
BATCH, ALPHA = 2, 0.5                                                 # toy networks; the HR side is 32: a tap of 8 x 8 = 64 points
H = HS.harness(350, BATCH)                                            # 64 channels, 2 blocks, LR 8 x 8, lr 5e-5


def test_step_with_the_term_on():
    from pesr_amd import contextual
    logs4, states4, calls = H.run(4, alpha_cx=ALPHA)
    logs0, states0, _ = H.run(2)
    assert calls == [{"taps": (contextual.TAP,)}] * 4
    got = logs4[0]["cx"]
    tr = H.trainer(alpha_cx=ALPHA)
    lr, hr = H.data()[0]
    with torch.no_grad():                                             # the sr of the first step: G before its update
        _, _, taps_sr, taps_hr = tr.vgg(tr.G(lr), hr, taps=(contextual.TAP,))
    assert tuple(taps_sr[0].shape) == (BATCH, 8, 8, 256)
    s = O.stages(taps_sr[0].cpu().numpy(), taps_hr[0].cpu().numpy(), H_BAND)
    want = float(s["L"].mean()) * ALPHA
    # an error e of CX relative to CX is an error e of L = -log CX; the mean and the weight are fp32
    allowed = ALPHA * CX_ALLOWED + 2.0 ** -22 * want
    print(f"logged cx term {got!r}, restated {want!r}, |difference| {abs(got - want):.3e}, allowed {allowed:.3e}; "
          f"m {float(s['m'].min()):.4f} .. {float(s['m'].max()):.4f}, CX {s['CX'].tolist()}")
    assert np.isfinite(got) and got > 0 and abs(got - want) <= allowed
    HS.assert_only_G_moved(logs4[0], states4[0], logs0[0], states0[0])


def test_step_with_texture_and_cx_calls_the_vgg_once_with_the_union():
    from pesr_amd import contextual
    both, _, calls = H.run(2, alpha_cx=ALPHA, alpha_texture=ALPHA, texture_patch=8)
    tex, _, calls_tex = H.run(2, alpha_texture=ALPHA, texture_patch=8)
    cx, _, _ = H.run(4, alpha_cx=ALPHA)
    assert calls == [{"taps": (1, 6, 11, contextual.TAP)}] * 2 and calls_tex == [{"taps": (1, 6, 11)}] * 2
    assert both[0]["texture"] == tex[0]["texture"] and both[0]["cx"] == cx[0]["cx"]      # the bits of the runs with one term
    for k in tex[0]:
        assert both[0][k] == tex[0][k], k
