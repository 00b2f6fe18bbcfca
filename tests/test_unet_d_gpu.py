"""GPU: the U-Net discriminator (--d_arch unet, docs/modes.md section 4v) - the bilinear x2 kernels and the logit-map GAN loss against
the float64 restatements of tests/unet_d_oracle.py, the module and two calls of it in one graph against float64 autograd, and train
steps (eager, captured, repeated, resumed) bit for bit; the default Discriminator's step is what it was."""
import numpy as np
import pytest
import torch

import unet_d_oracle as O
from helpers import dis_sd, gen_sd, vgg_sd
from oracle import detrand

pytestmark = pytest.mark.gpu

_SHARED = {}


# ---- 1. bilinear x2, forward and backward -----------------------------------------------------------------------------------------------
# the issue's shapes, and one with several channel blocks per pixel tile, a ragged last block and several ragged pixel tiles
UP_SHAPES = [(1, 1, 1, 4), (1, 1, 5, 4), (1, 5, 1, 4), (2, 3, 2, 8), (1, 5, 7, 3), (2, 6, 10, 64), (1, 9, 17, 132)]
_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("addend", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=_ids)
def test_up2_forward_against_float64_within_the_derived_bound(shape, addend):
    """|err| <= gamma(8) * sum |w_k| |in_k| + one ulp: four products and three adds in any order, fused or not, on inputs a + b that
    were rounded once (five roundings on any path; gamma(8) leaves room).  in_k = |a + b| in float64."""
    from pesr_amd import ops
    a, b = O.rand(shape, 1), (O.rand(shape, 2, 3.0) if addend else None)
    y = ops.bilinear_up2_fwd(a.cuda(), None if b is None else b.cuda()).cpu().double()
    s = a.double() + (b.double() if addend else 0.0)
    want = O.up2(s)
    assert y.shape == want.shape
    bound = O.gamma(8) * O.up2(s.abs()) + O.ulp32(want)
    err = (y - want).abs()
    print(f"up2 fwd {shape} addend={addend}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("shape", UP_SHAPES, ids=_ids)
def test_up2_backward_against_float64_within_the_derived_bound(shape):
    """|err| <= gamma(32) * sum |w_k| |gy_k| + one ulp: sixteen weighted terms in any order."""
    from pesr_amd import ops
    N, H, W, C = shape
    gy = O.rand((N, 2 * H, 2 * W, C), 3)
    gx = ops.bilinear_up2_bwd(gy.cuda()).cpu().double()
    want = O.up2_t(gy.double())
    assert gx.shape == want.shape == shape
    bound = O.gamma(32) * O.up2_t(gy.double().abs()) + O.ulp32(want)
    err = (gx - want).abs()
    print(f"up2 bwd {shape}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("shape", UP_SHAPES, ids=_ids)
def test_up2_backward_is_the_adjoint_of_the_forward(shape):
    """<up2(x), g> = <x, up2^T(g)> with both products summed in float64, to gamma(64) * sum |terms|: the backward is the adjoint of the
    forward kernel, not merely close to the reference's."""
    from pesr_amd import ops
    N, H, W, C = shape
    x, g = O.rand(shape, 4), O.rand((N, 2 * H, 2 * W, C), 5)
    y = ops.bilinear_up2_fwd(x.cuda()).cpu().double()
    gx = ops.bilinear_up2_bwd(g.cuda()).cpu().double()
    lhs, rhs = (y * g.double()), (x.double() * gx)
    tol = O.gamma(64) * float(lhs.abs().sum() + rhs.abs().sum())
    print(f"adjoint {shape}: |lhs - rhs| / tol = {abs(float(lhs.sum() - rhs.sum())) / tol:.3f}")
    assert abs(float(lhs.sum() - rhs.sum())) <= tol


def test_up2_node_returns_one_gradient_for_both_addends_and_the_same_bits_twice():
    from pesr_amd import functional as PF
    a, b = O.rand((2, 6, 10, 64), 6).cuda().requires_grad_(True), O.rand((2, 6, 10, 64), 7).cuda().requires_grad_(True)
    g = O.rand((2, 12, 20, 64), 8).cuda()
    y = PF.BilinearUp2Fn.apply(a, b)
    y.backward(g)
    assert torch.equal(a.grad, b.grad) and torch.equal(PF.BilinearUp2Fn.apply(a, b), y)
    a2 = a.detach().clone().requires_grad_(True)
    PF.BilinearUp2Fn.apply(a2, b.detach()).backward(g)
    assert torch.equal(a2.grad, a.grad)
    with pytest.raises(ValueError, match="bilinear_up2_fwd.b"):
        PF.BilinearUp2Fn.apply(a, b[:, :3])
    with pytest.raises(ValueError, match="bilinear_up2_bwd.gy"):
        from pesr_amd import ops
        ops.bilinear_up2_bwd(torch.zeros(1, 3, 4, 4).cuda())


# ---- 2. the GAN loss of a logit map -----------------------------------------------------------------------------------------------------
MAP_SIZES = [1, 1024, 1025, 2 * 24 * 24, 70001]           # 70001: 69 rows in the second stage (more than its 16 lanes), the last one ragged
MAP_CASES = [(g, 0, False, 1.0) for g in ("SGAN", "RSGAN", "RaSGAN")] + [(g, 1, False, 1.0) for g in ("SGAN", "RSGAN", "RaSGAN")] + \
            [(g, 1, True, gam) for g in ("SGAN", "RSGAN", "RaSGAN") for gam in (1.0, 2.0)]


def _logits(n, kind):
    """Standard-normal logits, or logits saturated at +-30 / +-90 with random signs.  A lone saturated pair is (-S, -S): with any other
    signs one of the twelve losses is log(1 + e^-S) alone, which fp32 cannot tell from 0 (1 + e^-30 rounds to 1) - a relative
    tolerance says nothing there, for these kernels as for ATen's fp32 ones; among many logits such terms vanish beside the O(S) ones."""
    r, f = O.rand((n,), 31), O.rand((n,), 32)
    if kind != "normal":
        S = 30.0 if kind == "sat30" else 90.0
        r, f = torch.sign(r) * S, torch.sign(f) * S
        if n == 1:
            r, f = torch.full((1,), -S), torch.full((1,), -S)
    return r, f


TINY32 = float(np.finfo(np.float32).tiny)      # below fp32's smallest normal number a result may be flushed to zero


@pytest.mark.parametrize("kind", ["normal", "sat30", "sat90"])
@pytest.mark.parametrize("n", MAP_SIZES)
def test_map_loss_against_float64(n, kind):
    """value rtol 1e-5; each gradient tensor within 1e-4 of the float64 maximum (each plus fp32's smallest normal number, below which a
    result may be flushed to zero); everything finite at saturated logits"""
    from pesr_amd import ops
    r, f = _logits(n, kind)
    rc, fc = r.cuda(), f.cuda()
    worst = [0.0, 0.0]
    for gan, side, focal, gam in MAP_CASES:
        out, d_r, d_f = ops.gan_loss_map(rc, fc, gan, side, focal, gam, 0.7)
        v, g_r, g_f = O.gan_loss(r.double(), f.double(), gan, side, focal, gam, 0.7)
        what = (n, kind, gan, side, focal, gam)
        assert bool(torch.isfinite(out).all() and torch.isfinite(d_r).all() and torch.isfinite(d_f).all()), what
        assert abs(float(out[0]) - float(v)) <= 1e-5 * abs(float(v)) + TINY32, (what, float(out[0]), float(v))
        worst[0] = max(worst[0], abs(float(out[0]) - float(v)) / max(abs(float(v)), 1e-300))
        for got, want in ((d_r, g_r), (d_f, g_f)):
            err, top = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
            assert err <= 1e-4 * top + TINY32, (what, err, top)
            worst[1] = max(worst[1], err / top if top else 0.0)
    if n == 1 and kind != "normal":      # the lone pairs of mixed sign: whatever fp32 makes of log(1 + e^-S), it is finite
        S = float(r.abs()[0])
        for sr_, sf_ in ((S, -S), (-S, S), (S, S)):
            pr, pf = torch.full((1,), sr_).cuda(), torch.full((1,), sf_).cuda()
            for gan, side, focal, gam in MAP_CASES:
                for t in ops.gan_loss_map(pr, pf, gan, side, focal, gam, 0.7):
                    assert bool(torch.isfinite(t).all()), (sr_, sf_, gan, side, focal, gam)
    print(f"map loss n={n} {kind}: worst value rel err {worst[0]:.2e}, worst gradient err / max {worst[1]:.2e}")


def test_map_loss_null_gradients_shapes_and_the_same_bits_twice():
    from pesr_amd import functional as PF, ops
    r, f = O.rand((2, 1, 24, 24), 33).cuda(), O.rand((2, 1, 24, 24), 34).cuda()
    for gan in ("SGAN", "RSGAN", "RaSGAN"):
        out, d_r, d_f = ops.gan_loss_map(r, f, gan, 1, True, 1.0, 1.0)
        out2, none, d_f2 = ops.gan_loss_map(r, f, gan, 1, True, 1.0, 1.0, need_real=False)
        assert none is None and torch.equal(out, out2) and torch.equal(d_f, d_f2) and d_f.shape == f.shape
        out3, d_r3, none = ops.gan_loss_map(r, f, gan, 1, True, 1.0, 1.0, need_fake=False)
        assert none is None and torch.equal(out, out3) and torch.equal(d_r, d_r3)
    rr, ff = r.clone().requires_grad_(True), f.clone().requires_grad_(True)
    (2.0 * PF.gan_loss(rr, ff, "RaSGAN", 0)).backward()
    _, d_r, d_f = ops.gan_loss_map(r, f, "RaSGAN", 0, False, 1.0, 1.0)
    assert torch.equal(rr.grad, d_r * 2.0) and torch.equal(ff.grad, d_f * 2.0)
    with pytest.raises(ValueError, match="gan_loss_map.pred_fake"):
        ops.gan_loss_map(r, f[:1], "SGAN", 0, False, 1.0)
    with pytest.raises(ValueError, match="gan_loss_map.gan_type"):
        ops.gan_loss_map(r, f, "WGAN", 0, False, 1.0)
    with pytest.raises(ValueError, match="gan_loss_map.pred_real"):
        ops.gan_loss_map(r[:0], f[:0], "SGAN", 0, False, 1.0)


@pytest.mark.parametrize("B", [1, 16, 1024])
def test_batch_logits_up_to_1024_still_run_the_old_kernel(B, monkeypatch):
    from pesr_amd import functional as PF, ops
    r, f = O.rand((B, 1), 35).cuda().requires_grad_(True), O.rand((B, 1), 36).cuda().requires_grad_(True)
    want = {g: ops.gan_loss(r.detach(), f.detach(), g, 1, True, 1.0, 0.5) for g in ("SGAN", "RSGAN", "RaSGAN")}
    monkeypatch.setattr(ops, "gan_loss_map", lambda *a, **k: pytest.fail("the map kernel ran on [B, 1] logits"))
    for g, (out, d_r, d_f) in want.items():
        r.grad = f.grad = None
        loss = PF.gan_loss(r, f, g, 1, True, 1.0, 0.5)
        loss.backward()
        assert torch.equal(loss.detach(), out[0]) and torch.equal(r.grad, d_r) and torch.equal(f.grad, d_f), g


def test_a_longer_vector_of_logits_runs_the_map_kernel():
    from pesr_amd import functional as PF
    r, f = O.rand((1025, 1), 37), O.rand((1025, 1), 38)
    got = PF.gan_loss(r.cuda(), f.cuda(), "RaSGAN", 0)
    want = O.gan_loss(r.double(), f.double(), "RaSGAN", 0)[0]
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))


# ---- 3. conv9 (C -> 1) and the module -----------------------------------------------------------------------------------------------------
def _ratio(got, want):
    """max |got - want| over the float64 maximum of want"""
    err, top = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
    return err / top if top else (0.0 if err == 0.0 else float("inf"))


def _within(got, want, what, tol=1e-4):
    err, top = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
    assert err <= tol * top + 1e-300, (what, err, top)
    return err / top if top else 0.0


@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (1, 5, 19, 16), (2, 33, 17, 132)], ids=_ids)
def test_conv_to_one_channel_against_float64(shape):
    """forward, input gradient and weight gradient of the logit layer's own kernels (the routed 3 x 3 path refuses Cout = 1 backward)"""
    from pesr_amd import ops
    import torch.nn.functional as F
    N, H, W, C = shape
    x, w, b, g = O.rand(shape, 41), O.rand((1, C, 3, 3), 42, 0.1), O.rand((1,), 43), O.rand((N, H, W, 1), 44)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, b64, padding=1)
    y64.backward(g.double().permute(0, 3, 1, 2))
    y = ops.conv3x3_c1_fwd(x.cuda(), w.cuda(), b.cuda())
    m = [_within(y, y64.detach().permute(0, 2, 3, 1), "y"),
         _within(ops.conv3x3_c1_dgrad(g.cuda(), w.cuda(), shape), x64.grad.permute(0, 2, 3, 1), "dx")]
    dw, db = ops.conv3x3_c1_wgrad(x.cuda(), g.cuda())
    m += [_within(dw, w64.grad, "dw"), _within(db, b64.grad, "db")]
    dw2, none = ops.conv3x3_c1_wgrad(x.cuda(), g.cuda(), want_bias=False)
    assert none is None and torch.equal(dw, dw2)
    print(f"conv C->1 {shape}: err / max of y, dx, dw, db = " + ", ".join(f"{v:.2e}" for v in m))


def _unet(sn, seed=0, w=64):
    from pesr_amd.model import UNetDiscriminator
    state = torch.random.get_rng_state()
    torch.manual_seed(900 + seed)
    D = UNetDiscriminator({"spectral_norm": sn, "d_width": w})
    torch.random.set_rng_state(state)
    return D.cuda()


@pytest.mark.parametrize("sn", [False, True], ids=["plain", "sn"])
@pytest.mark.parametrize("size", [(16, 16), (24, 40)], ids=_ids)
def test_module_against_float64(size, sn):
    """logits, every parameter gradient and the input gradient within 1e-4 of the float64 maximum (the tolerance tests/test_model_gpu.py
    states for gradients); conv9 with Cout = 1 is pinned here"""
    D = _unet(sn)
    sd = O.leaves(D)
    x = detrand.image_batch((2, 3) + size, 71)
    g = O.rand((2, 1) + size, 72)
    xc = x.cuda().requires_grad_(True)
    y = D(xc)
    assert y.shape == (2, 1) + size
    (y * g.cuda()).sum().backward()
    x64 = x.double().requires_grad_(True)
    y64 = O.unet_d(sd, x64)
    (y64 * g.double()).sum().backward()
    rows = {"logits": _within(y, y64.detach(), "logits"), "input": _within(xc.grad, x64.grad, "input")}
    for k, p in D.named_parameters():
        rows[k] = _within(p.grad, sd[k].grad, k)
    if sn:       # the power iteration moved u and v as the float64 one did
        for k in ("conv1.weight_u", "conv8.weight_v"):
            _within(D.state_dict()[k], sd[k].detach(), k)
    print(f"module {size} sn={sn}: worst err / max = {max(rows.values()):.2e} ({max(rows, key=rows.get)}); logits {rows['logits']:.2e}")


def test_module_refuses_a_size_that_is_no_multiple_of_8():
    D = _unet(False, w=16)
    with pytest.raises(ValueError, match=r"\(1, 3, 12, 16\)"):
        D(torch.zeros(1, 3, 12, 16).cuda())


# ---- 4. two calls in one graph --------------------------------------------------------------------------------------------------------
def _pair(seeds=(81, 82)):
    return detrand.image_batch((2, 3, 16, 16), seeds[0]), detrand.image_batch((2, 3, 16, 16), seeds[1])


def _one_graph(gan, sn, seeds=(81, 82)):
    """-> (float64 gradient of every parameter with its two contributions - out of D(hr) and out of D(sr) -, the product's gradients,
    how close the float64 forward comes to a kink of a LeakyReLU: the smallest |pre-activation| over its layer's maximum)"""
    from pesr_amd import functional as PF
    D = _unet(sn, 1)
    sd = O.leaves(D)
    hr, sr = _pair(seeds)
    loss = PF.gan_loss(D(hr.cuda()), D(sr.cuda()), gan, 0)
    loss.backward()
    kinks = []
    r64, f64 = O.unet_d(sd, hr.double(), kinks=kinks), O.unet_d(sd, sr.double(), kinks=kinks)
    loss64 = O.gan_loss_autograd(r64, f64, gan, 0)
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    names = [k for k, _ in D.named_parameters()]
    g_r, g_f = torch.autograd.grad(loss64, [r64, f64], retain_graph=True)
    use_r = torch.autograd.grad(r64, [sd[k] for k in names], g_r, retain_graph=True)
    use_f = torch.autograd.grad(f64, [sd[k] for k in names], g_f)
    got = {k: p.grad.detach().cpu().double() for k, p in D.named_parameters()}
    return {k: (a + b, a, b) for k, a, b in zip(names, use_r, use_f)}, got, min(kinks)


def _one_graph_rows(gan, sn, seeds):
    want, got, kink = _one_graph(gan, sn, seeds)
    rows = {}
    for k, (total, a, b) in want.items():
        top = float(total.abs().max())
        if k == "conv9.bias" and gan != "SGAN":
            top = max(float(a.abs().max()), float(b.abs().max()))
        rows[k] = float((got[k] - total).abs().max()) / top
    print(f"one graph {gan} sn={sn} images {seeds}: closest pre-activation to a kink {kink:.1e} of its layer's maximum; worst err / max = "
          f"{max(rows.values()):.2e} ({max(rows, key=rows.get)}); all: " + ", ".join(f"{k} {v:.1e}" for k, v in rows.items()))
    return rows, kink


@pytest.mark.parametrize("gan, sn", [("SGAN", False), ("RSGAN", False), ("RaSGAN", False), ("SGAN", True)])
def test_discriminator_loss_of_two_calls_in_one_graph_against_float64(gan, sn):
    """D(hr), D(sr), the discriminator's loss, one backward: every parameter gradient is the sum of two uses, within 1e-4 of its float64
    maximum.  One tensor has no maximum to be relative to: the relativistic losses do not change when every logit moves by the same
    amount, so conv9.bias's gradient - the sum of all logit gradients - is exactly zero, as the difference of the two uses'
    contributions (float64 leaves 6e-17, fp32 6e-8).  It is held to 1e-4 of the larger of those two contributions instead."""
    rows, _ = _one_graph_rows(gan, sn, (81, 82))
    assert max(rows.values()) <= 1e-4, rows


KINK_CLEARANCE = 2e-6


@pytest.mark.parametrize("gan", ["RSGAN", "RaSGAN"])
def test_relativistic_loss_of_two_calls_under_spectral_norm_against_float64(gan):
    """The relativistic losses with spectral norm, the same 1e-4 of the float64 maximum.  The images are another seeded pair than above, and
    why is asserted: a LeakyReLU's gradient jumps at zero, so where a float64 pre-activation lies within fp32's resolution of zero an
    fp32 forward may land on the other side, and from that one element on the two gradients are those of different functions.  With the
    pair (81, 82) and spectral norm one pre-activation of conv6 in the first call is 5e-8 of the layer's maximum (below fp32's 6e-8), the
    kernels' forward has the other sign at exactly that element, and they gave conv6.weight_orig to 2.5e-4 and the layers in front of it to 5e-5 - 8e-5, the layers behind it and the whole
    second call to 5e-7 - 2e-6, where torch's own fp32 evaluation on the CPU, which happened to land on float64's side, stays at 2.4e-6.
    The pair (112, 113) keeps every pre-activation of both calls at least 3.4e-6 of its layer's maximum away from zero, above the
    KINK_CLEARANCE this test requires and several times the kernels' forward error (1e-6 of the maximum on the logits)."""
    rows, kink = _one_graph_rows(gan, True, (112, 113))
    assert kink >= KINK_CLEARANCE, kink
    assert max(rows.values()) <= 1e-4, rows


@pytest.mark.parametrize("gan", ["SGAN", "RSGAN", "RaSGAN"])
@pytest.mark.parametrize("focal", [False, True], ids=["bce", "focal"])
def test_generator_side_gradient_of_sr_against_float64(gan, focal):
    from pesr_amd import functional as PF
    D = _unet(False, 2)
    sd = {k: v.detach() for k, v in O.leaves(D).items()}
    for p in D.parameters():
        p.requires_grad = False
    hr, sr = _pair()
    src = sr.cuda().requires_grad_(True)
    pred_fake = D(src)
    with torch.no_grad():
        pred_real = D(hr.cuda())
    loss = PF.gan_loss(pred_real, pred_fake, gan, 1, focal, 1.0, 0.5)
    loss.backward()
    sr64 = sr.double().requires_grad_(True)
    loss64 = O.gan_loss_autograd(O.unet_d(sd, hr.double()).detach(), O.unet_d(sd, sr64), gan, 1, focal, 1.0, 0.5)
    loss64.backward()
    assert abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64))
    print(f"generator side {gan} focal={focal}: err / max = {_within(src.grad, sr64.grad, 'sr'):.2e}")
    assert all(p.grad is None for p in D.parameters())


# ---- 5. train steps ---------------------------------------------------------------------------------------------------------------------
CH, DEPTH, PS, BATCH, LR = 64, 2, 8, 2, 5e-5


def _vgg():
    if "vgg" not in _SHARED:
        from model import VGG
        V = VGG(); V.load_state_dict(vgg_sd()); V.cuda()
        _SHARED["vgg"] = V
    return _SHARED["vgg"]


def _data():
    if "data" not in _SHARED:
        _SHARED["data"] = [(detrand.image_batch((BATCH, 3, PS, PS), 350 + i).cuda(),
                            detrand.image_batch((BATCH, 3, 4 * PS, 4 * PS), 360 + i).cuda()) for i in range(4)]
    return _SHARED["data"]


def _trainer(seed=0, sn=True, gan_type="SGAN", D=None):
    """SGAN by default: under the relativistic losses conv9.bias's gradient is exactly zero (a shift of every logit changes nothing),
    and the first test below wants to see every parameter of D move."""
    from model import Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = Generator({"num_channels": CH, "depth": DEPTH, "res_scale": 0.1, "scale": 4})
    G.load_state_dict(gen_sd(CH, DEPTH, seed)); G.cuda()
    D = _unet(sn, 10 + seed) if D is None else D
    return Trainer(G, D, _vgg(), FlatAdam(G.parameters(), lr=LR, betas=(0.9, 0.999)), FlatAdam(D.parameters(), lr=LR, betas=(0.9, 0.999)),
                   gan_type=gan_type)


def _state(tr):
    return {"G": tr.optim_G.flat.flat_p.clone(), "G.exp_avg": tr.optim_G.exp_avg.clone(), "D": tr.optim_D.flat.flat_p.clone(),
            "D.exp_avg": tr.optim_D.exp_avg.clone(), **{"D." + k: v.clone() for k, v in tr.D.state_dict().items()}}


def _logs(d):
    return {k: v.item() for k, v in d.items()}


def _four_eager():
    if "eager" not in _SHARED:
        tr = _trainer()
        start = {k: v.detach().clone() for k, v in tr.D.named_parameters()}
        logs, states = [], []
        for lr, hr in _data():
            logs.append(_logs(tr.gan_step(lr, hr)))
            states.append(_state(tr))
        _SHARED["eager"] = (logs, states, start, {k: v.detach().clone() for k, v in tr.D.named_parameters()})
    return _SHARED["eager"]


def _assert_state(tr, want, what):
    got = _state(tr)
    assert sorted(got) == sorted(want)
    for k in got:
        assert torch.equal(got[k], want[k]), (what, k)


def test_two_eager_steps_are_finite_and_move_every_parameter_of_d():
    logs, states, start, end = _four_eager()
    assert set(logs[0]) == {"l1", "vgg", "g", "tv", "d"}
    assert all(np.isfinite(v) for l in logs[:2] for v in l.values()), logs[:2]
    assert len(start) == 12          # ten weights, two biases
    for k in start:
        assert not torch.equal(start[k], end[k]) and bool(torch.isfinite(end[k]).all()), k


def test_two_eager_steps_a_capture_and_two_replays_are_four_eager_steps():
    logs4, states4, _, _ = _four_eager()
    tr = _trainer()
    data = _data()
    for i in range(2):
        assert _logs(tr.gan_step(*data[i])) == logs4[i]
    step = tr.capture_gan_step(*data[0])
    for i in (2, 3):
        assert _logs(step(*data[i])) == logs4[i], i
        _assert_state(tr, states4[i], f"replay {i}")


def test_a_second_run_gives_the_same_bits():
    logs4, states4, _, _ = _four_eager()
    tr = _trainer()
    for i, (lr, hr) in enumerate(_data()[:2]):
        assert _logs(tr.gan_step(lr, hr)) == logs4[i]
        _assert_state(tr, states4[i], f"second run, step {i + 1}")


@pytest.mark.parametrize("gan_type", ["RSGAN", "RaSGAN"])
def test_the_other_gan_types_step_too(gan_type):
    tr = _trainer(gan_type=gan_type, sn=False)
    logs = [_logs(tr.gan_step(lr, hr)) for lr, hr in _data()[:2]]
    assert all(np.isfinite(v) for l in logs for v in l.values()), logs


def test_resume_after_two_steps_equals_four_uninterrupted(tmp_path):
    from pesr_amd import checkpoint
    logs4, states4, _, _ = _four_eager()
    tr = _trainer()
    data = _data()
    for lr, hr in data[:2]:
        tr.gan_step(lr, hr)
    path = str(tmp_path / "state.pt")
    checkpoint.atomic_save({"G": tr.G.state_dict(), "D": tr.D.state_dict(), "optim_G": tr.optim_G.state_dict(),
                            "optim_D": tr.optim_D.state_dict()}, path)
    st = checkpoint.load_state(path)
    assert "conv9.bias" in st["D"] and "conv1.weight_u" in st["D"]
    fresh = _trainer(seed=40)              # other weights, zero moments
    assert not torch.equal(fresh.optim_D.flat.flat_p, states4[1]["D"])
    fresh.G.load_state_dict(st["G"]); fresh.D.load_state_dict(st["D"])
    fresh.optim_G.load_state_dict(st["optim_G"]); fresh.optim_D.load_state_dict(st["optim_D"])
    for i in (2, 3):
        assert _logs(fresh.gan_step(*data[i])) == logs4[i], i
        _assert_state(fresh, states4[i], f"resumed, step {i + 1}")


def test_new_kernels_do_not_depend_on_the_precision_mode():
    from pesr_amd import ops
    a, b, g = O.rand((2, 6, 10, 64), 91).cuda(), O.rand((2, 6, 10, 64), 92).cuda(), O.rand((2, 12, 20, 64), 93).cuda()
    r, f = O.rand((2, 1, 24, 24), 94).cuda(), O.rand((2, 1, 24, 24), 95).cuda()
    w, d1 = O.rand((1, 64, 3, 3), 96).cuda(), O.rand((2, 6, 10, 1), 97).cuda()

    def run():
        return [ops.bilinear_up2_fwd(a, b), ops.bilinear_up2_bwd(g), *ops.gan_loss_map(r, f, "RaSGAN", 1, True, 1.0, 1.0),
                ops.conv3x3_c1_fwd(a, w, None), ops.conv3x3_c1_dgrad(d1, w, a.shape), ops.conv3x3_c1_wgrad(a, d1)[0]]
    want = run()
    with ops.use_precision("bf16"):
        got = run()
    assert all(torch.equal(x, y) for x, y in zip(got, want))


# ---- 6. the default ---------------------------------------------------------------------------------------------------------------------
def test_default_discriminator_step_is_what_it_was():
    """A Trainer whose D was built with no new argument and one whose D came through d_arch="vgg": the same logs over two steps, bit for
    bit, and the logits are [B, 1]: the old loss kernel."""
    from pesr_amd.model import Discriminator, build_discriminator
    opt = {"patch_size": PS, "spectral_norm": False}

    def made(make):
        D = make(); D.load_state_dict(dis_sd(PS, 1)); D.cuda()
        tr = _trainer(D=D)
        return [_logs(tr.gan_step(lr, hr)) for lr, hr in _data()[:2]], tr
    a, tr = made(lambda: Discriminator(opt))
    b, _ = made(lambda: build_discriminator(opt))
    c, _ = made(lambda: build_discriminator(dict(opt, d_width=64), d_arch="vgg"))
    assert a == b == c and all(np.isfinite(v) for l in a for v in l.values())
    assert type(tr.D) is Discriminator and tr.D(_data()[0][1]).shape == (BATCH, 1)
