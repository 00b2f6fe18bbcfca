"""GPU: the x2 / x3 extension of --scale (docs/modes.md section 4e) on the HIP kernels - the standalone r = 2 / 3 PixelShuffle
kernels, the x2 / x3 Generator against the float64 restatement of tests/scale_oracle.py, the x3 upsampler at the dispatch of a
real run, the Discriminator and VGG at the HR sizes x2 / x3 bring (96 and 144), GAN / pretrain steps against oracle.step, the
captured step and the entry points.  Tolerances follow tests/test_model_gpu.py's header."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import adam_close, close, dis_sd, vgg_sd
from oracle import detrand
from oracle import model as OM
from oracle import step as OS
from scale_oracle import ScaledTrainState, gen_sd_scaled, generator_forward_scaled

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message=".*pretrained vgg19.*")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leaf(t, dt):
    """A fresh leaf copy of t in dtype dt (t.to(dt) returns t itself, with its accumulated .grad, when the dtype already matches)."""
    return t.detach().to(dt).clone().requires_grad_(True)


def _max_rel(a, b, mx):
    a, b = (np.asarray(t.detach().cpu(), dtype=np.float64) for t in (a, b))
    return float(np.abs(a - b).max()) / mx


def _grads_gv4b(ours, g64, g32, what=""):
    """GV4b's criterion (helpers.grads_vs_fp64) with the float32 side computed here on the CPU: per tensor, the maximum error of
    our gradient against float64 is at most 3x the CPU float32 error of that tensor, and never has to beat twice the worst CPU
    float32 error of any tensor of the network (a flipped ReLU / LeakyReLU decision is a discrete event, so one tensor's own float32
    error is a one-sample estimate).  ours / g64 / g32: {name: tensor}."""
    rows = {}
    for k in g64:
        mx = float(g64[k].abs().max())
        if mx == 0.0:
            continue
        rows[k] = (_max_rel(ours[k], g64[k], mx), _max_rel(g32[k], g64[k], mx))
    net_floor = max(r[1] for r in rows.values())
    for k, (e, e_ref) in rows.items():
        tol = max(3.0 * e_ref, 2.0 * net_floor, 1e-6)
        assert e <= tol, f"{what}grad {k}: error vs fp64 {e:.2e} > {tol:.2e} (CPU fp32 {e_ref:.2e}, network floor {net_floor:.2e})"
    return rows, net_floor


def _G(C, depth, scale, sd):
    from model import Generator
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1, "scale": scale})
    G.load_state_dict(sd)
    return G.cuda()


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 1), (2, 5, 7, 1), (3, 7, 5, 3), (2, 9, 11, 16), (2, 13, 5, 256), (1, 3, 50, 64)])
def test_pixel_shuffle_r_bit_exact(r, N, H, W, C):
    from pesr_amd import ops
    x = torch.randn(N, H, W, r * r * C, device="cuda")
    y = ops.pixel_shuffle_r_fwd(x, r)
    ref = F.pixel_shuffle(x.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
    assert y.shape == (N, r * H, r * W, C) and torch.equal(y, ref)
    assert torch.equal(ops.pixel_shuffle_r_fwd(x, r), y)                        # deterministic
    dy = torch.randn(N, r * H, r * W, C, device="cuda")
    dx = ops.pixel_shuffle_r_bwd(dy, r)
    assert torch.equal(dx, F.pixel_unshuffle(dy.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1))
    assert torch.equal(ops.pixel_shuffle_r_bwd(dy, r), dx)
    if r == 2:                                                                   # the old r = 2 entry points, bit for bit
        assert torch.equal(ops.pixel_shuffle_fwd(x), y) and torch.equal(ops.pixel_shuffle_bwd(dy), dx)


def test_pixel_shuffle_r_refuses_other_factors():
    from pesr_amd import _lib, ops
    x = torch.zeros(1, 2, 2, 16, device="cuda")
    L = _lib.lib()
    y = torch.empty(1, 8, 8, 1, device="cuda")
    assert L.pesr_pixel_shuffle_r_fwd(x.data_ptr(), y.data_ptr(), 1, 2, 2, 1, 4, ops._stream()) == -1
    assert L.pesr_pixel_shuffle_r_bwd(y.data_ptr(), x.data_ptr(), 1, 2, 2, 1, 1, ops._stream()) == -1
    with pytest.raises(_lib.PesrHipError):
        ops.pixel_shuffle_r_fwd(x, 4)


def test_pixel_shuffle_r3_above_2_pow_31_elements():
    """One tensor of 2.15e9 elements (64-bit offsets): the round trip is exact and the last image rows - offsets above 2^31 -
    equal torch's shuffle of the matching input rows, compared on the device."""
    from pesr_amd import ops
    N, H, W, C, r = 1, 966, 966, 256, 3
    assert N * H * W * r * r * C > 2 ** 31
    x = torch.rand(N, H, W, r * r * C, device="cuda")
    y = ops.pixel_shuffle_r_fwd(x, r)
    tail = 4
    ref = F.pixel_shuffle(x[:, H - tail:].permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
    assert torch.equal(y[:, r * (H - tail):], ref)
    ref0 = F.pixel_shuffle(x[:, :tail].permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
    assert torch.equal(y[:, :r * tail], ref0)
    del ref, ref0
    dx = ops.pixel_shuffle_r_bwd(y, r)
    assert torch.equal(dx, x)


# ---------------------------------------------------------------------------------------------------------------- Generator
@pytest.mark.parametrize("scale", [2, 3])
@pytest.mark.parametrize("C", [16, 64])
def test_generator_small_fwd_bwd_vs_oracle(scale, C):
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    sd = gen_sd_scaled(C, 2, scale)
    G = _G(C, 2, scale, sd)
    lr = detrand.image_batch((2, 3, 12, 12), 1234)
    hr = detrand.image_batch((2, 3, 12 * scale, 12 * scale), 1235)
    sr = G(lr.cuda())
    assert sr.shape == (2, 3, 12 * scale, 12 * scale)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = generator_forward_scaled(sd64, lr.double(), 2, 0.1, scale)
    close(sr, ref, 1e-5, 2e-3, "sr")
    loss = PF.l1_loss(nhwc(sr), nhwc(hr.cuda().contiguous(memory_format=torch.channels_last)))
    loss_ref = F.l1_loss(ref, hr.double())
    close(loss, loss_ref, 1e-5, what="l1")
    loss.backward(); loss_ref.backward()
    for k, p in G.named_parameters():
        close(p.grad, sd64[k].grad, 1e-4, what="grad " + k)


@pytest.mark.parametrize("scale", [2, 3])
def test_generator_ragged_image_and_x8_ensemble(scale):
    import importlib.util
    from oracle import image as OI
    spec = importlib.util.spec_from_file_location("entry_test_scale", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    sd = gen_sd_scaled(16, 2, scale, seed=5)
    G = _G(16, 2, scale, sd)
    img = detrand.image_batch((1, 3, 13, 22), 77)
    with torch.no_grad():
        out = G(img.cuda())
        ref = generator_forward_scaled(sd, img, 2, 0.1, scale)
        close(out, ref, 1e-5, 2e-3, "ragged")
        ens = T.x8_forward(img.cuda(), G)
        ens_ref = OI.x8_forward(img, lambda t: generator_forward_scaled(sd, t, 2, 0.1, scale))
    assert ens.shape == (1, 3, 13 * scale, 22 * scale)
    close(ens, ens_ref, 1e-5, 2e-3, "x8")


def test_x3_upsampler_at_real_dispatch(monkeypatch):
    """C = 256, B = 16, LR 48, depth 1: the upsampler conv 256 -> 2304 forward and input gradient on F(4,3), its weight gradient
    on the default wgrad path (algo 0, F(4,3) first), the r = 3 shuffle both ways; values of images 0 and 15 against float64
    (only their outputs enter the loss, so the CPU side stays affordable while every kernel runs at the full batch)."""
    from pesr_amd import _lib, ops
    C, B, S = 256, 16, 48
    assert ops.wino4_eligible(B, S, S, C, 9 * C) and ops._wg4_plan_ok(B, S, S, C, 9 * C) == (True, 1)
    kname = ops.wgrad_kernel_for(B, S, S, C, 9 * C)[0]
    assert kname.startswith("conv3x3_wgrad_wino4") and kname == ops.wgrad_kernel_for(B, S, S, C, C)[0]   # the G body's kernel
    sd = gen_sd_scaled(C, 1, 3, seed=9)
    G = _G(C, 1, 3, sd)
    n = {"F43": 0, "wgrad_9C": 0, "shuffle_fwd": 0, "shuffle_bwd": 0}
    inner = ops._conv3x3_wino

    def counted(x, wp, bias, skip, mask, y, N, H, W, cin, cout, *a, **k):
        if isinstance(wp, ops.Wino4Packed) and 9 * C in (cin, cout):      # upsample.0 forward (256 -> 2304) and dgrad (2304 -> 256)
            n["F43"] += 1
        return inner(x, wp, bias, skip, mask, y, N, H, W, cin, cout, *a, **k)
    monkeypatch.setattr(ops, "_conv3x3_wino", counted)
    L = _lib.lib()

    class _Shim:
        def __getattr__(s, name):
            f = getattr(L, name)
            if name == "pesr_conv3x3_wgrad":
                def g(*args):
                    if args[8] == 9 * C and args[7] == C:
                        n["wgrad_9C"] += 1
                        assert args[12] == 0                      # the default algorithm choice
                    return f(*args)
                return g
            if name in ("pesr_pixel_shuffle_r_fwd", "pesr_pixel_shuffle_r_bwd"):
                def h(*args):
                    n["shuffle_" + name[-3:]] += 1
                    return f(*args)
                return h
            return f
    monkeypatch.setattr(_lib, "lib", lambda: _Shim())
    lr = detrand.image_batch((B, 3, S, S), 4321)
    gw = detrand.uniform((2, 3, 3 * S, 3 * S), 4322)
    sr = G(lr.cuda())
    loss = (sr[[0, B - 1]] * gw.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert n["shuffle_fwd"] == 1 and n["shuffle_bwd"] == 1, n
    assert n["F43"] == 2, n                       # forward + input gradient of upsample.0 on F(4,3)
    assert n["wgrad_9C"] == 1, n
    refs = {}
    for dt in (torch.float64, torch.float32):
        sdr = {k: _leaf(v, dt) for k, v in sd.items()}
        ref = generator_forward_scaled(sdr, lr[[0, B - 1]].to(dt), 1, 0.1, 3)
        (ref * gw.to(dt)).sum().backward()
        refs[dt] = (sdr, ref)
    close(sr[[0, B - 1]], refs[torch.float64][1], 1e-5, 2e-3, "sr")
    # GV4b's criterion on the tensors behind the trunk's last ReLU - the upsampler's and add_mean's - whose gradients take no
    # decision; the trunk in front is the x4 trunk (test_fullsize_gpu GV2b), where a flipped ReLU moves a weight gradient as a whole
    keys = [k for k in sd if k.startswith(("upsample.", "add_mean."))]
    params = dict(G.named_parameters())
    _grads_gv4b({k: params[k].grad for k in keys}, {k: refs[torch.float64][0][k].grad for k in keys},
                {k: refs[torch.float32][0][k].grad for k in keys}, "upsampler x3: ")


# ---------------------------------------------------------------------------------------------------------------- D and VGG
@pytest.mark.parametrize("hr_size,scale", [(96, 2), (144, 3)])
def test_discriminator_at_hr_size_vs_oracle(hr_size, scale):
    from model import Discriminator
    B, ps = 16, hr_size // scale
    d_sd = dis_sd(hr_size // 4)
    D = Discriminator({"patch_size": ps, "spectral_norm": False, "scale": scale})
    D.load_state_dict(d_sd)
    D = D.cuda()
    a = detrand.image_batch((B, 3, hr_size, hr_size), 21)
    b = detrand.image_batch((B, 3, hr_size, hr_size), 22)
    bg = b.cuda().requires_grad_(True)
    dec = [_d_gpu_decisions(D, a), _d_gpu_decisions(D, b)]       # before the calls: BatchNorm normalises by batch statistics
    o1, o2 = D(a.cuda()), D(bg)
    l = F.binary_cross_entropy_with_logits(o1 - o2, torch.ones(B, 1, device="cuda"))
    l.backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sdr = {k: (_leaf(v, dt) if v.is_floating_point() and not OS.is_buffer(k) else v.detach().to(dt).clone() if v.is_floating_point()
                   else v.clone()) for k, v in d_sd.items()}
        br = _leaf(b, dt)
        r1, r2 = OM.discriminator_forward(sdr, a.to(dt)), OM.discriminator_forward(sdr, br)
        lr_ = F.binary_cross_entropy_with_logits(r1 - r2, torch.ones(B, 1, dtype=dt))
        lr_.backward()
        refs[dt] = (sdr, br, r1, r2, lr_)
    sd64, b64, r1, r2, lr_ = refs[torch.float64]
    sd32, b32 = refs[torch.float32][:2]
    close(o1, r1, 5e-5, what="o1"); close(o2, r2, 5e-5, what="o2"); close(l, lr_, 2e-5, what="bce")
    # Every LeakyReLU is a decision that fp32 rounding can take the other way; the plain float64 comparison counts such flips as
    # errors.  So the gradients are held to GV4b's criterion (grads_vs_fp64: 3x the float32 error, or twice the network's worst) on a
    # float64 / CPU float32 restatement that takes the GPU's own LeakyReLU decisions (the signs of each block's and the hidden
    # layer's outputs) - on every element - and the flips are counted.
    gd = {}
    for dt in (torch.float64, torch.float32):
        sdr = {k: (_leaf(v, dt) if v.is_floating_point() and not OS.is_buffer(k) else v.detach().to(dt).clone() if v.is_floating_point()
                   else v.clone()) for k, v in d_sd.items()}
        br = _leaf(b, dt)
        q1, q2 = _d_forward_with_decisions(sdr, a.to(dt), dec[0]), _d_forward_with_decisions(sdr, br, dec[1])
        F.binary_cross_entropy_with_logits(q1 - q2, torch.ones(B, 1, dtype=dt)).backward()
        gd[dt] = (sdr, br)
    params = {k: p.grad for k, p in D.named_parameters()}
    g64 = {k: gd[torch.float64][0][k].grad for k in params}
    g64["input"] = gd[torch.float64][1].grad
    g32 = {k: gd[torch.float32][0][k].grad for k in params}
    g32["input"] = gd[torch.float32][1].grad
    rows, _ = _grads_gv4b(dict(params, input=bg.grad), g64, g32, f"D at {hr_size} (GPU decisions): ")
    flips = sum(_d_flips(d_sd, x, dd) for x, dd in ((a, dec[0]), (b, dec[1])))
    e_plain = _max_rel(bg.grad, b64.grad, float(b64.grad.abs().max()))
    print(f"D {hr_size}: {flips} LeakyReLU decisions differ from float64's; input gradient error vs fp64 {e_plain:.2e}, "
          f"vs fp64 with the GPU's decisions {rows['input'][0]:.2e} (CPU fp32 with them {rows['input'][1]:.2e})")
    for k, v in D.state_dict().items():
        if "running" in k:
            close(v, sd64[k], 1e-4, what=k)
        elif "num_batches" in k:
            assert int(v) == 2
    # classify_pair is bit for bit two separate classify() calls at this width
    with torch.no_grad():
        fa, fb = D.forward_features(a.cuda()), D.forward_features(b.cuda())
        pa, pb = D.classify_pair(fa, fb)
        assert torch.equal(pa, D.classify(fa)) and torch.equal(pb, D.classify(fb))
    assert fa.shape == (B, 512 * (hr_size // 16) ** 2)


@pytest.mark.parametrize("size", [96, 144])
def test_vgg_at_hr_size(size):
    from model import VGG
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    v_sd = vgg_sd()
    V = VGG(); V.load_state_dict(v_sd); V = V.cuda()
    x = detrand.image_batch((2, 3, size, size), 41)
    y = detrand.image_batch((2, 3, size, size), 42)
    res = []
    for merged in (True, False):
        a = x.cuda().requires_grad_(True)
        if not merged:
            V.TAIL_START = 10 ** 6
        try:
            fa, fb = V(a, y.cuda())
        finally:
            V.TAIL_START = type(V).TAIL_START
        assert fa.shape == (2, 512, size // 16, size // 16)
        PF.mse_loss(nhwc(fa), nhwc(fb)).backward()
        res.append((fa.detach().clone(), fb.clone(), a.grad.clone()))
    close(res[0][0], res[1][0], 1e-5, what="features(sr)")
    close(res[0][1], res[1][1], 1e-5, what="features(hr)")
    close(res[0][2], res[1][2], 2e-5, what="d mse / d sr")
    x64 = x.double().requires_grad_(True)
    f_sr, f_hr = OM.vgg_forward({k: t.double() for k, t in v_sd.items()}, x64, y.double())
    close(res[1][0], f_sr, 2e-5, what="f_sr vs fp64"); close(res[1][1], f_hr, 2e-5, what="f_hr vs fp64")
    F.mse_loss(f_sr, f_hr).backward()
    # The input gradient crosses 15 ReLU kinks and 4 max-pool argmaxes: one decision taken the other way by fp32 rounding moves the
    # gradient of the pixels behind it by up to their own size (the reference's own fp32 error at 192 is 2.7 % of the maximum,
    # tests/golden/gv7b_fp64.npz).  So the check takes the GPU's decisions - every ReLU mask and max-pool argmax of the separate-pass
    # forward - into a float64 (and a CPU float32) restatement: against it our gradient must be as close as fp32 arithmetic allows,
    # on every element, and the distance to the plain float64 gradient must come from decisions alone.
    dec, flips = _vgg_gpu_decisions(V, x, v_sd)
    gd = {}
    for dt in (torch.float64, torch.float32):
        xr = _leaf(x, dt)
        fs = _vgg_features_with_decisions({k: t.to(dt) for k, t in v_sd.items()}, xr, dec)
        F.mse_loss(fs, res[1][1].cpu().to(dt)).backward()        # the GPU's own hr features as the target
        gd[dt] = xr.grad
    mx = float(gd[torch.float64].abs().max())
    e_dec, f_dec = _max_rel(res[1][2], gd[torch.float64], mx), _max_rel(gd[torch.float32], gd[torch.float64], mx)
    e_plain = _max_rel(res[1][2], x64.grad, float(x64.grad.abs().max()))
    print(f"VGG {size}: {flips} decisions differ from float64's; input gradient error vs fp64 {e_plain:.2e}, "
          f"vs fp64 with the GPU's decisions {e_dec:.2e} (CPU fp32 with them {f_dec:.2e})")
    assert e_dec <= max(3.0 * f_dec, 1e-6), f"grad input vs fp64 with the GPU's decisions: {e_dec:.2e} > 3 x {f_dec:.2e}"
    assert flips > 0 or e_plain <= max(3.0 * f_dec, 1e-6)


def _d_gpu_decisions(D, x):
    """Signs (> 0) of the GPU Discriminator's block outputs and hidden layer for input x, from a copy of D run block by block as
    forward_features chains them (the copy keeps D's running statistics untouched)."""
    import copy
    from pesr_amd import functional as PF
    from pesr_amd import ops
    Dc = copy.deepcopy(D)
    out, flat, link = [], x.cuda(), None
    with torch.no_grad():
        for blk in Dc.features:
            flat, link = blk.forward_linked(flat, link)
            out.append((flat > 0).cpu().contiguous())
        flat = flat.view(flat.size(0), -1)
        fc1, act, _ = Dc.classifier
        out.append((PF.LinearFn.apply(flat, fc1.weight, fc1.bias, ops.ACT_LRELU, act.negative_slope, None) > 0).cpu())
    return out


def _d_forward_with_decisions(sd, x, dec):
    """oracle.model.discriminator_forward (no running-stat update) with each LeakyReLU's side taken from `dec`."""
    h = x
    for i, (_, _, stride) in enumerate(OM.discriminator_plan()):
        h = F.conv2d(h, sd[f"features.{i}.0.weight"], None, stride=stride, padding=1)
        h = F.batch_norm(h, None, None, sd[f"features.{i}.1.weight"], sd[f"features.{i}.1.bias"], True, 0.1, 1e-5)
        h = torch.where(dec[i], h, 0.2 * h)
    h = F.linear(h.reshape(h.size(0), -1), sd["classifier.0.weight"], sd["classifier.0.bias"])
    h = torch.where(dec[-1], h, 0.2 * h)
    return F.linear(h, sd["classifier.2.weight"], sd["classifier.2.bias"])


def _d_flips(d_sd, x, dec):
    """How many of the GPU's LeakyReLU decisions differ from the float64 forward's."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d_sd.items()}
    n, h = 0, x.double()
    with torch.no_grad():
        for i, (_, _, stride) in enumerate(OM.discriminator_plan()):
            h = F.conv2d(h, sd[f"features.{i}.0.weight"], None, stride=stride, padding=1)
            h = F.batch_norm(h, None, None, sd[f"features.{i}.1.weight"], sd[f"features.{i}.1.bias"], True, 0.1, 1e-5)
            n += int(((h > 0) != dec[i]).sum())
            h = F.leaky_relu(h, 0.2)
        h = F.linear(h.reshape(h.size(0), -1), sd["classifier.0.weight"], sd["classifier.0.bias"])
        n += int(((h > 0) != dec[-1]).sum())
    return n


def _vgg_gpu_decisions(V, x, v_sd):
    """The GPU VGG's ReLU masks (output > 0 of every conv + ReLU) and max-pool argmaxes (first maximum in scan order, as the pool
    kernel's backward recomputes it), from a step-by-step run of the separate-pass forward; and how many of them differ from the
    float64 forward's."""
    from pesr_amd import ops
    dec, h, prev = [], None, False
    with torch.no_grad():
        h = V.sub_mean(x.cuda())
        for kind, m, has_relu in V._steps(0, len(V.vgg)):
            if kind == "conv":
                h = m(h, act=ops.ACT_RELU if has_relu else ops.ACT_NONE, relu_in=prev, relu_grad_by_consumer=has_relu)
                prev = has_relu
                if has_relu:
                    dec.append(("relu", (h > 0).cpu().contiguous()))
            else:
                dec.append(("pool", F.max_pool2d(h.cpu().contiguous(), 2, 2, return_indices=True)[1]))
                h = m(h, relu_in=prev)
                prev = False
    # the same decisions of the float64 forward
    flips, it = 0, iter(dec)
    sd64 = {k: t.double() for k, t in v_sd.items()}
    with torch.no_grad():
        h = F.conv2d(x.double(), sd64["sub_mean.weight"], sd64["sub_mean.bias"])
        idx = 0
        for v in OM.VGG_CFG_E:
            if idx >= 35:
                break
            if v == "M":
                _, ind = next(it)
                h, ind64 = F.max_pool2d(h, 2, 2, return_indices=True)
                flips += int((ind64 != ind).sum())
                idx += 1
            else:
                h = F.conv2d(h, sd64[f"vgg.{idx}.weight"], sd64[f"vgg.{idx}.bias"], padding=1)
                idx += 1
                if idx < 35:
                    _, mask = next(it)
                    h = F.relu(h)
                    flips += int(((h > 0) != mask).sum())
                idx += 1
    return dec, flips


def _vgg_features_with_decisions(sd, x, dec):
    """oracle.model.vgg_features with each ReLU's mask and each max-pool's argmax taken from `dec` instead of from its own values."""
    it = iter(dec)
    h = F.conv2d(x, sd["sub_mean.weight"], sd["sub_mean.bias"])
    idx = 0
    for v in OM.VGG_CFG_E:
        if idx >= 35:
            break
        if v == "M":
            _, ind = next(it)
            N, C, H, W = h.shape
            h = h.reshape(N, C, H * W).gather(2, ind.reshape(N, C, -1)).reshape(N, C, H // 2, W // 2)
            idx += 1
        else:
            h = F.conv2d(h, sd[f"vgg.{idx}.weight"], sd[f"vgg.{idx}.bias"], padding=1)
            idx += 1
            if idx < 35:
                _, mask = next(it)
                h = h * mask.to(h.dtype)
            idx += 1
    return h


# ---------------------------------------------------------------------------------------------------------------- train steps
def _trainer(C, depth, scale, ps, g_sd, d_sd, v_sd, lr=5e-5, **kw):
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1, "scale": scale}); G.load_state_dict(g_sd); G.cuda()
    D = Discriminator({"patch_size": ps, "spectral_norm": False, "scale": scale}); D.load_state_dict(d_sd); D.cuda()
    V = VGG(); V.load_state_dict(v_sd); V.cuda()
    return Trainer(G, D, V, FlatAdam(G.parameters(), lr=lr), FlatAdam(D.parameters(), lr=lr), **kw), G, D


@pytest.mark.parametrize("scale,gp", [(2, False), (3, False), (3, True)])
def test_gan_step_vs_oracle(scale, gp):
    LR = 16
    HR = LR * scale
    g_sd, d_sd, v_sd = gen_sd_scaled(64, 1, scale), dis_sd(HR // 4), vgg_sd()
    tr, G, D = _trainer(64, 1, scale, LR, g_sd, d_sd, v_sd, alpha_l1=0.5, gradient_penalty=gp)
    st = ScaledTrainState(g_sd, d_sd, v_sd, {"depth": 1, "res_scale": 0.1, "learning_rate": 5e-5, "alpha_l1": 0.5, "scale": scale,
                                             "GP": gp})
    lr = detrand.image_batch((4, 3, LR, LR), 500); hr = detrand.image_batch((4, 3, HR, HR), 501)
    if gp:
        u = detrand.uniform((4, 1, 1, 1), 502, 0.0, 1.0)
        ref = OS.gan_step(st, lr, hr, gp_u=u)
        log = tr.gan_step(lr.cuda(), hr.cuda(), gp_u=u.cuda())
    else:
        ref = OS.gan_step(st, lr, hr)
        log = tr.gan_step(lr.cuda(), hr.cuda())
    for k in ("l1", "vgg", "g", "tv", "d"):
        assert float(log[k]) == pytest.approx(ref[k], rel=5e-5, abs=1e-7), k
    for k, v in G.state_dict().items():
        adam_close(v, st.g[k], 5e-5, 1, "G." + k)
    for k, v in D.state_dict().items():
        if v.is_floating_point() and not OS.is_buffer(k):
            adam_close(v, st.d[k], 5e-5, 1, "D." + k)


def test_pretrain_step_x3_vs_oracle():
    from model import Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    g_sd = gen_sd_scaled(64, 2, 3)
    G = Generator({"num_channels": 64, "depth": 2, "res_scale": 0.1, "scale": 3}); G.load_state_dict(g_sd); G.cuda()
    tr = Trainer(G, None, None, FlatAdam(G.parameters(), lr=1e-4), None)
    st = ScaledTrainState(g_sd, None, None, {"depth": 2, "res_scale": 0.1, "learning_rate": 1e-4, "scale": 3})
    for i in range(2):
        lr = detrand.image_batch((4, 3, 12, 12), 600 + i); hr = detrand.image_batch((4, 3, 36, 36), 610 + i)
        ref = OS.pretrain_step(st, lr, hr)
        log = tr.pretrain_step(lr.cuda(), hr.cuda())
        assert float(log["l1"]) == pytest.approx(ref["l1"], rel=2e-5)
    for k, v in G.state_dict().items():
        adam_close(v, st.g[k], 1e-4, 2, "G." + k)


def test_gan_step_x3_hipgraph_replay_is_bit_identical_to_eager():
    g_sd, d_sd, v_sd = gen_sd_scaled(16, 2, 3), dis_sd(12), vgg_sd()        # LR 16 -> HR 48
    tra, Ga, Da = _trainer(16, 2, 3, 16, g_sd, d_sd, v_sd)
    trb, Gb, Db = _trainer(16, 2, 3, 16, g_sd, d_sd, v_sd)
    data = [(detrand.image_batch((4, 3, 16, 16), 50 + i).cuda(), detrand.image_batch((4, 3, 48, 48), 60 + i).cuda()) for i in range(4)]
    for lr, hr in data[:2]:
        tra.gan_step(lr, hr); trb.gan_step(lr, hr)
    step = trb.capture_gan_step(*data[0])
    for lr, hr in data[2:]:
        la, lb = tra.gan_step(lr, hr), step(lr, hr)
        for k in la:
            assert la[k].item() == lb[k].item(), k
    for pa, pb in zip(list(Ga.parameters()) + list(Da.parameters()), list(Gb.parameters()) + list(Db.parameters())):
        assert torch.equal(pa, pb)


# ---------------------------------------------------------------------------------------------------------------- entry points
def _png_folder(root, scale, sizes, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    for sub in ("LR", "HR"):
        (root / sub).mkdir(parents=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(root / "LR" / f"{i}.png")
        Image.fromarray(rng.randint(0, 256, (scale * h, scale * w, 3)).astype(np.uint8)).save(root / "HR" / f"{i}.png")


def test_train_entrypoint_x3(tmp_path):
    """train.py --scale 3, both phases, host loader (synthetic) and --gpu_pipeline (PNG folder), in a fresh interpreter."""
    _png_folder(tmp_path / "data" / "origin" / "train" / "Toy", 3, [(20, 24)] * 4, 1)
    _png_folder(tmp_path / "data" / "origin" / "valid" / "Toy", 3, [(12, 10)], 2)
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
def common(ck, extra):
    return ["--scale", "3", "--num_channels", "16", "--num_blocks", "1", "--patch_size", "16", "--batch_size", "4",
            "--num_epochs", "1", "--max_iters", "2", "--check_point", ck, "--snapshot_every", "1"] + extra
syn = ["--synthetic", "8"]
gpu = ["--train_dataset", "Toy", "--valid_dataset", "Toy", "--num_repeats", "2", "--gpu_pipeline", "true", "--allow_random_vgg", "true"]
Tm.main(common({ck!r} + "/syn", syn + ["--phase", "pretrain"]))
best = os.path.join({ck!r}, "syn", "pretrain", "best_model.pt")
Tm.main(common({ck!r} + "/syn", syn + ["--phase", "train", "--pretrained_model", best]))
Tm.main(common({ck!r} + "/gpu", gpu + ["--phase", "pretrain"]))
Tm.main(common({ck!r} + "/gpu", gpu + ["--phase", "train", "--pretrained_model", best]))
print("ENTRY_OK")
"""
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    from pesr_amd.model import scale_of_state_dict
    for run in ("syn", "gpu"):
        sd = torch.load(tmp_path / "ck" / run / "train" / "model_1.pt", map_location="cpu")
        assert scale_of_state_dict(sd) == 3 and all(bool(torch.isfinite(v).all()) for v in sd.values())


def test_gpu_patch_sampler_x3_bit_exact():
    import random
    from data import augment
    from pesr_amd.input_pipeline import GpuPatchSampler
    rng = np.random.RandomState(3)
    lrs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((20, 17), (11, 30))]
    hrs = [rng.randint(0, 256, (3 * l.shape[0], 3 * l.shape[1], 3)).astype(np.uint8) for l in lrs]
    samp = GpuPatchSampler(lrs, hrs, torch.device("cuda"), scale=3)
    P = 7
    picks = samp.draw(8, P, random.Random(5))
    for nhwc in (False, True):
        lr, hr = samp.assemble(picks, P, nhwc=nhwc)
        assert lr.shape == (8, 3, P, P) and hr.shape == (8, 3, 3 * P, 3 * P)
        for b, (i, y, x, aug) in enumerate(picks):
            l = lrs[i][y:y + P, x:x + P]
            h = hrs[i][3 * y:3 * (y + P), 3 * x:3 * (x + P)]
            l, h = augment(l, h, aug)
            assert torch.equal(lr[b].cpu(), torch.from_numpy(l.transpose(2, 0, 1).astype(np.float32)))
            assert torch.equal(hr[b].cpu(), torch.from_numpy(h.transpose(2, 0, 1).astype(np.float32)))


def test_test_entrypoint_x3(tmp_path, monkeypatch):
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("entry_test_x3", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    lr_dir = tmp_path / "data" / "origin" / "test" / "Toy" / "LR"
    lr_dir.mkdir(parents=True)
    arr = detrand.image_batch((17, 14, 3), 901).numpy().astype(np.uint8)
    Image.fromarray(arr).save(lr_dir / "a.png")
    sd = gen_sd_scaled(16, 1, 3, seed=3)
    torch.save(sd, tmp_path / "g3.pt")
    T.main(["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g3.pt"), "--num_channels", "16", "--num_blocks", "1",
            "--scale", "3", "--save_path", str(tmp_path / "out")])
    got = np.asarray(Image.open(tmp_path / "out" / "Toy" / "a.png").convert("RGB")).astype(np.int32)
    from oracle import image as OI
    with torch.no_grad():
        want = OI.tensor_to_img(generator_forward_scaled(sd, torch.from_numpy(arr.transpose(2, 0, 1)[None].astype(np.float32)), 1, 0.1, 3))
    assert got.shape == want.shape == (51, 42, 3)
    assert np.abs(got - want.astype(np.int32)).max() <= 1
    with pytest.raises(SystemExit, match="x3 generator, but --scale is 4"):
        T.main(["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g3.pt"), "--num_channels", "16", "--num_blocks", "1"])
