"""CPU: tests/streaming_oracle.py itself against torch autograd and torch.optim on inputs small enough to read.  This is where the tie
semantics that tests/test_streaming_gpu.py holds the kernels to are pinned to ATen: the first maximum of a pooling window in row-major
order, sign(0) = 0, and "not > 0 takes the slope" at 0.0 and at -0.0."""
import pytest
import torch
import torch.nn.functional as F

import streaming_oracle as SO
from oracle import step as OS


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("relu_in", [True, False])
@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 14, 14, 64)])
def test_maxpool_backward_sends_the_gradient_to_atens_winner_at_ties(shape, relu_in):
    x = SO.tied_pool_input(shape, 5).double()
    tied, windows = SO.maxpool_tied_windows(x)
    assert 3 * tied >= windows, (tied, windows)                    # 93 of 240 and 1387 of 3136
    assert bool(((x == 0) & torch.signbit(x)).any())                # the -0.0 is there
    dy = torch.randn(shape[0], shape[1] // 2, shape[2] // 2, shape[3], generator=torch.Generator().manual_seed(6)).double()
    xr = _nchw(x).clone().requires_grad_(True)
    F.max_pool2d(torch.relu(xr) if relu_in else xr, 2, 2).backward(_nchw(dy))
    assert torch.equal(_nchw(SO.maxpool_bwd(x, dy, relu_in)), xr.grad)
    assert torch.equal(_nchw(SO.maxpool_fwd(x)), F.max_pool2d(_nchw(x), 2, 2))


@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (1, 3, 2, 4)])
def test_maxpool_forward_is_floor_mode_on_odd_sides(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).double()
    assert torch.equal(_nchw(SO.maxpool_fwd(x)), F.max_pool2d(_nchw(x), 2, 2))


def test_l1_tv_value_and_gradient_with_equal_pixels_and_equal_neighbours():
    sr, hr = (t.double() for t in SO.tied_images((2, 9, 11, 3), 3))
    assert int((sr == hr).sum()) * 10 >= sr.numel()
    assert int((sr[:, :, :-1] == sr[:, :, 1:]).sum()) * 10 >= sr.numel()
    g_l1, g_tv = 0.3 / sr.numel(), 1e-3
    s = _nchw(sr).clone().requires_grad_(True)
    l1, tv = F.l1_loss(s, _nchw(hr)), OS.tv_loss(s)
    (0.3 * l1 + 1e-3 * tv).backward()
    val = SO.l1_tv_value(sr, hr)
    assert float(val[0]) == pytest.approx(float(l1.detach()), rel=1e-14) and float(val[1]) == pytest.approx(float(tv.detach()), rel=1e-14)
    grad = SO.l1_tv_grad(sr, hr, g_l1, g_tv)
    assert float((_nchw(grad) - s.grad).abs().max()) <= 1e-15       # products of a few units in the last place of 1e-3
    # and the count of signs alone, exactly: d(tv)/d(sr) is an integer
    s2 = _nchw(sr).clone().requires_grad_(True)
    OS.tv_loss(s2).backward()
    assert torch.equal(_nchw(SO.tv_sign_count(sr)), s2.grad)
    a = torch.randn(2, 5, 6, 4, dtype=torch.double, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    b = torch.randn(2, 5, 6, 4, dtype=torch.double, generator=torch.Generator().manual_seed(4))
    m = F.mse_loss(a, b)
    (50 * m).backward()
    assert float(SO.mse_value(a.detach(), b)) == pytest.approx(float(m.detach()), rel=1e-14)
    assert float((SO.mse_grad(a.detach(), b, 50 * 2.0 / a.numel()) - a.grad).abs().max()) <= 1e-15


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_relu_mask_at_both_zeros_is_atens_leaky_relu_backward(slope):
    z = torch.tensor([-2.0, -0.0, 0.0, 3.0, 0.0, -0.0, 1e-30, -1e-30], dtype=torch.double)
    g = torch.tensor([1.0, 2.0, 3.0, 4.0, -5.0, -6.0, 7.0, 8.0], dtype=torch.double)
    zr = z.clone().requires_grad_(True)
    (F.leaky_relu(zr, slope) if slope else F.relu(zr)).backward(g)
    out = SO.relu_mask(g, z, None, 1.0, slope)
    assert torch.equal(out, zr.grad)
    assert torch.equal(out[1:3], slope * g[1:3])                    # slope * g (0 for ReLU) at 0.0 and at -0.0
    # the forward of a LeakyReLU is the same expression with the input as its own reference, the scaled add has no reference
    assert torch.equal(SO.relu_mask(z, z, None, 1.0, slope), F.leaky_relu(z, slope))
    assert torch.equal(SO.relu_mask(g, None, z, 0.5), 0.5 * g + z)
    assert torch.equal(SO.relu_mask(g, None, None, 0.5), 0.5 * g)
    assert torch.equal(SO.relu_mask(g, z, g, 0.5, slope), torch.where(z > 0, 0.5 * g, slope * 0.5 * g) + g)


def test_meanshift_is_a_1x1_conv():
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(2, 5, 7, 3, dtype=torch.double, generator=gen) * 255
    w = torch.eye(3, dtype=torch.double) + torch.rand(3, 3, dtype=torch.double, generator=gen) * 0.1
    b = torch.rand(3, dtype=torch.double, generator=gen) * 100
    dy = torch.randn(2, 5, 7, 3, dtype=torch.double, generator=gen)
    xr, wr, br = _nchw(x).clone().requires_grad_(True), w.view(3, 3, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br)
    y.backward(_nchw(dy))
    assert float((_nchw(SO.meanshift_fwd(x, w, b)) - y.detach()).abs().max()) <= 1e-12
    dx, dw, db = SO.meanshift_bwd(dy, x, w)
    assert float((_nchw(dx) - xr.grad).abs().max()) <= 1e-13
    assert float((dw - wr.grad.view(3, 3)).abs().max()) <= 1e-9 and float((db - br.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_adam_oracle_is_torch_optim_adam(gscale):
    """Three steps in float64; torch gets the gradient already scaled."""
    lr, b1, b2, eps = 5e-5, 0.9, 0.999, 1e-8
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(300, dtype=torch.double, generator=gen)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        g = (torch.randn(300, generator=gen) * 3)                   # fp32, as the kernels get it
        q.grad = g.double() * gscale
        opt.step()
        p, m, v = SO.adam_step(p, m, v, g, b1, b2, eps, *SO.adam_scalars(lr, b1, b2, step), gscale)
        st = opt.state[q]
        assert float((m - st["exp_avg"]).abs().max()) <= 1e-15 and float((v - st["exp_avg_sq"]).abs().max()) <= 1e-15
        assert float((p - q.detach()).abs().max()) <= 1e-15, step  # |p| ~ 1: a few units in the last place
    assert float((p - torch.randn(300, dtype=torch.double, generator=torch.Generator().manual_seed(11))).abs().max()) > 1e-5   # it moved


@pytest.mark.parametrize("gan_type,side,focal,gamma", SO.GAN_CASES)
def test_gan_loss_oracle_in_fp32_is_the_inline_reference_of_test_ops_gpu(gan_type, side, focal, gamma):
    """The expressions test_gan_loss_kernel_vs_oracle computes inline (tests/test_ops_gpu.py), on its own inputs at B = 16."""
    gen = torch.Generator().manual_seed(7)
    B = 16
    r = (torch.randn(B, 1, generator=gen) * 4).requires_grad_(True)
    f = (torch.randn(B, 1, generator=gen) * 4).requires_grad_(True)
    with torch.no_grad():
        r[0] = 30.0; f[1] = -40.0; r[2] = -25.0
    ones, zeros = torch.ones(B, 1), torch.zeros(B, 1)
    bce = F.binary_cross_entropy_with_logits
    lf = (lambda z, t: OS.focal_loss(z, t, gamma)) if focal else bce
    if side == 0:
        ref = {"SGAN": lambda: bce(r, ones) + bce(f, zeros), "RSGAN": lambda: bce(r - f, ones),
               "RaSGAN": lambda: 0.5 * (bce(r - f.mean(), ones) + bce(f - r.mean(), zeros))}[gan_type]()
    else:
        ref = {"SGAN": lambda: lf(f, ones), "RSGAN": lambda: lf(f - r, ones),
               "RaSGAN": lambda: 0.5 * (lf(r - f.mean(), zeros) + lf(f - r.mean(), ones))}[gan_type]()
    (ref * 0.7).backward()
    val, d_r, d_f = SO.gan_loss_and_grads(r.detach(), f.detach(), gan_type, side, focal, gamma, 0.7)
    assert val.dtype == torch.float32 and float(val) == float((ref * 0.7).detach())
    assert torch.equal(d_f, f.grad)
    assert torch.equal(d_r, r.grad if r.grad is not None else torch.zeros_like(r))
    # and in float64 it is the same function: the fp32 value lies within fp32 rounding of it
    val64, _, _ = SO.gan_loss_and_grads(r.detach().double(), f.detach().double(), gan_type, side, focal, gamma, 0.7)
    assert val64.dtype == torch.float64 and float(val64) == pytest.approx(float(val), rel=1e-5, abs=1e-9)
