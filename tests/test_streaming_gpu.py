"""GPU: the HBM-bound kernels that every train step runs - adam.hip, elementwise.hip (MeanShift, PixelShuffle, relu_mask, 2x2 max-pool),
loss.hip (L1 + TV, MSE, PSNR-Y, GAN loss) - against tests/streaming_oracle.py in float64 (docs/experiments/streaming_tests.md).

Each of them is `for (e = tid; e < total; e += gridDim * blockDim)` under a fixed or capped grid of 256-thread blocks.  Sizes follow that
geometry - the smallest that make the loop go round a second time and stop at a ragged end:

    kernel                                   items per pass                    size here
    adam_kernel, adam_dev_kernel             8192 * 256 = 2 097 152 float4     2^21 + 1 and 5 * 2^20 + 3 float4 (and 257)
    relu_mask                                2 097 152 float4                  2^21 + 300 float4
    maxpool_fwd / bwd                        2 097 152 output float4           1 x 2050 x 2050 x 8: 2 101 250
    pixel_shuffle                            2 097 152 scalars                 1 x 363 x 365 x 16: 2 119 920
    meanshift_fwd                            4096 * 256 = 1 048 576 pixels     2 x 725 x 725: 1 051 250
    meanshift_bwd, l1_tv                     1024 * 256 = 262 144 pixels       2 x 363 x 362: 262 812
    mse                                      512 * 256 = 131 072 float4        2 x 23 x 23 x 512: 135 424
    psnr_y                                   256 * 256 = 65 536 pixels         257 x 256: 65 792
    gan_loss                                 one block of 16 waves             B = 1, 63, 64, 65, 1000, 1024

Error bounds count fp32 roundings, u = 2^-24 each (round to nearest; hipcc's fp32 division and square root are correctly rounded), k of
them in a row compounding to (1 + u)^k - 1.  A fused multiply-add makes one rounding where the count assumes two, so the bounds hold
whichever way the compiler contracts.  Each test prints its worst error / bound before it asserts."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import streaming_oracle as SO
from oracle import detrand
from oracle import ops as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D = 2.0 ** -40        # far above anything the kernels' double-precision sums (a few thousand additions at 2^-53) can lose


def _k(n):
    """n fp32 roundings in a row."""
    return (1.0 + U) ** n - 1.0


def _f32(x):
    """A Python float as the C ABI's `float` argument receives it."""
    return float(np.float32(x))


def _worst(err, bound, what):
    """max err / bound over float64 tensors, asserted <= 1 (where the bound is 0 the error must be 0; a NaN fails)."""
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f}"
    return worst


def _ulp(t):
    """Spacing of fp32 at |t| (float64 tensor)."""
    a = t.abs()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


def _passes(items, per_pass):
    return -(-items // per_pass)


# ================================================================================================
# Adam
# ================================================================================================
ADAM_SIZES = [4 * 257, 4 * ((1 << 21) + 1), 4 * (5 * (1 << 20) + 3)]
LR, B1, B2, EPS, GSCALE = _f32(5e-5), _f32(0.9), _f32(0.999), _f32(1e-8), 0.5
# 1 - b1 and 1 - b2 are exact in fp32 (b >= 0.5 is a multiple of 2^-24, and so is 1 - b, which is smaller), so the kernels' fp32
# constants are the float64 oracle's.


def _adam_buffers(n, seed, steps):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 1e-2                        # non-zero first moment
    v = torch.rand(n, generator=gen) * 1e-3 + 1e-6                  # positive second moment
    return p.cuda(), m.cuda(), v.cuda(), [torch.randn(n, generator=gen).cuda() for _ in range(steps)]


def _check_adam(tag, before, after, g, step_size, bc2_sqrt, scalar_roundings):
    """p, m, v after one step against the float64 oracle fed the fp32 state before it.  u = 2^-24, G = gscale * g, c1 = 1 - b1:

    m' = m + (G - m) c1: four roundings - G (u |G|), the difference (u |G - m| <= 2 u M with M = max(|m|, |G|)), the product, the sum
        (|m'| <= M).  The first three are scaled by c1 on their way into m':  c1 (1 + 2 + 2) u M + u M = (1 + 5 c1) u M, c_m = 1 + 5 c1 = 1.5.
        Products of two of the four errors: fewer than 16 pairs, factor (1 + 16 u).
    v' = v b2 + G G c2, all terms >= 0: G (u), G G (2 u + u), times c2 (u), v b2 (u), the sum (u): the longer chain is 5 roundings,
        c_v = 5, |dv| <= ((1 + u)^5 - 1) v'.
    p' = p - s m' / (sqrt(v') / q + eps): m' and v' are checked above against the state before the step, so here the oracle is fed the
        kernel's own fp32 m', v' and only the update's roundings remain: sqrt, the division by q, + eps, m' / den, times s (5), the
        roundings of s and q to fp32 where the host makes them (scalar_roundings = 2; 0 when the oracle is given the rounded scalars),
        and the subtraction, u |p'| <= u (|p| + |update|), whose second half counts as one more on the update:
        |dp| <= u |p| + ((1 + u)^c_p - 1) |s m' / den|, c_p = 5 + scalar_roundings + 1 = 8 (6 for the device-state form)."""
    (p0, m0, v0), (p1, m1, v1) = before, after
    p0, m0, v0 = p0.cpu().double(), m0.cpu().double(), v0.cpu().double()
    p1, m1, v1, g = p1.cpu(), m1.cpu(), v1.cpu(), g.cpu()
    m_ref, v_ref = SO.adam_moments(m0, v0, g, B1, B2, GSCALE)
    c_m = 1.0 + 5.0 * (1.0 - B1)
    big = torch.maximum(m0.abs(), (g.double() * GSCALE).abs())
    rm = _worst((m1.double() - m_ref).abs(), c_m * U * (1 + 16 * U) * big, f"{tag} m")
    rv = _worst((v1.double() - v_ref).abs(), _k(5) * v_ref, f"{tag} v")
    p_ref, upd, _ = SO.adam_param(p0, m1.double(), v1.double(), step_size, bc2_sqrt, EPS)
    rp = _worst((p1.double() - p_ref).abs(), U * p0.abs() + _k(6 + scalar_roundings) * upd.abs(), f"{tag} p")
    assert float(upd.abs().max()) > 0.1 * step_size and not torch.equal(m1.double(), m0)        # the step did something
    return rm, rv, rp


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_step_p_m_v_against_float64(n):
    """adam_kernel, two steps with gscale = 0.5 from a non-zero m and a positive v; the bounds are derived in _check_adam."""
    from pesr_amd import ops
    p, m, v, grads = _adam_buffers(n, 100 + n % 1000, 2)
    for step in (1, 2):
        g = grads[step - 1]
        g_keep = g.clone()
        before = (p.clone(), m.clone(), v.clone())
        ops.adam_step(p, g, m, v, LR, B1, B2, EPS, step, GSCALE)
        assert torch.equal(g, g_keep), "the gradient buffer was written"
        _check_adam(f"adam n {n} step {step}", before, (p, m, v), g, *SO.adam_scalars(LR, B1, B2, step), 2)


def _bits(x):
    return int(np.float32(x).view(np.int32))


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_step_dev_counter_scalars_and_update_against_float64(n):
    """adam_tick_kernel + adam_dev_kernel.  The step count lives in state[4..5] as two 32-bit halves: it is set through the int32 view so
    that the ticks land on 1, 2, 1000 and on 0xFFFFFFFF -> 2^32, the carry into state[5] (the two large sizes: 1 and 2^32), and the
    learning rate in state[0] changes between the calls.  After each tick state[2..3] hold float32(lr / bc1) and float32(sqrt(bc2)) of
    numpy float64 within one fp32 ulp (the device's pow need not be the host's); at 2^32 both corrections are 1.  p, m, v meet the
    bounds of _check_adam with the scalars the kernel read, which the oracle gets as they are (no rounding of theirs to count)."""
    from pesr_amd import ops
    ticks = (1, 2, 1000, 1 << 32) if n == ADAM_SIZES[0] else (1, 1 << 32)
    p, m, v, grads = _adam_buffers(n, 200 + n % 1000, len(ticks))
    st = torch.zeros(6, device="cuda")
    count = st.view(torch.int32)
    for i, t in enumerate(ticks):
        lr = _f32(LR * (1.0 + 0.5 * i))
        st[0] = lr
        prev = t - 1
        count[4] = (prev & 0xFFFFFFFF) - (1 << 32 if prev & 0x80000000 else 0)
        count[5] = prev >> 32
        g = grads[i]
        g_keep = g.clone()
        before = (p.clone(), m.clone(), v.clone())
        ops.adam_step_dev(p, g, m, v, st, B1, B2, EPS, GSCALE)
        assert torch.equal(g, g_keep), "the gradient buffer was written"
        got = st.cpu()
        halves = [int(x) & 0xFFFFFFFF for x in count.cpu()[4:6]]
        assert halves == [t & 0xFFFFFFFF, t >> 32], (t, halves)
        assert float(got[0]) == lr
        step_size, bc2_sqrt = SO.adam_scalars(lr, B1, B2, t)
        if t == 1 << 32:
            assert step_size == lr and bc2_sqrt == 1.0
        d2, d3 = _bits(float(got[2])) - _bits(step_size), _bits(float(got[3])) - _bits(bc2_sqrt)
        print(f"adam_dev n {n} tick {t}: state[2] {float(got[2]):.9e} (host {step_size:.9e}, {d2:+d} ulp), "
              f"state[3] {float(got[3]):.9e} (host {bc2_sqrt:.9e}, {d3:+d} ulp), bit-equal: {d2 == 0 and d3 == 0}")
        assert abs(d2) <= 1 and abs(d3) <= 1
        _check_adam(f"adam_dev n {n} tick {t}", before, (p, m, v), g, float(got[2]), float(got[3]), 0)


# ================================================================================================
# L1 + TV
# ================================================================================================
L1_N, L1_H, L1_W = 2, 363, 362                                     # 262 812 pixels: the image boundary n = 0 -> 1 falls mid-grid
G_L1, G_TV = _f32(0.3 / (L1_N * L1_H * L1_W * 3)), _f32(1e-3)


def _l1_tv_sum_bounds(sr64, hr64):
    """The two fp32 sums, relative to the sum of the absolute terms.  A term of the L1 sum passes through: its own subtraction (1), the
    thread's running sum - passes x 3 channels additions -, 6 butterfly steps of the wave sum, 3 additions of the four waves; then the
    partials are added in double and the result is stored as fp32 (1).  A pixel adds two TV terms per channel: passes x 3 x 2."""
    passes = _passes(L1_N * L1_H * L1_W, 1024 * 256)
    assert passes == 2
    a, h, v = SO.l1_tv_terms(sr64, hr64)
    k_l1, k_tv = 1 + passes * 3 + 6 + 3 + 1, 1 + passes * 3 * 2 + 6 + 3 + 1           # 17 and 23
    return (_k(k_l1) + D) * float(a.sum()) / a.numel(), (_k(k_tv) + D) * float(h.sum() + v.sum())


def _l1_tv_grad_fp32(sr, hr, g_l1, g_tv):
    """The gradient takes few values: g_l1 {-1, 0, 1} + g_tv {-4 .. 4}.  fp32 subtraction of fp32 numbers never gives 0 or the wrong sign
    unless they are equal, so the signs are those of float64; what is left is one product and one sum, which the compiler may or may not
    fuse: -> (unfused, fused), the kernel must be one of the two throughout.  (fused: product and sum are exact in float64 - 24 + 3 bits
    against 24 bits some 13 binades below - and rounded once.)"""
    s, t = torch.sign(sr - hr), SO.tv_sign_count(sr)
    gl, gt = torch.tensor(g_l1, dtype=torch.float32), torch.tensor(g_tv, dtype=torch.float32)
    return gl * s + gt * t, (gl.double() * s.double() + gt.double() * t.double()).float()


def _check_l1_tv(sr, hr, tag):
    from pesr_amd import ops
    out, grad = ops.loss_l1_tv(sr.cuda(), hr.cuda(), G_L1, G_TV)
    out2, none = ops.loss_l1_tv(sr.cuda(), hr.cuda(), G_L1, G_TV, need_grad=False)
    assert none is None and torch.equal(out, out2)
    ref = SO.l1_tv_value(sr.double(), hr.double())
    b_l1, b_tv = _l1_tv_sum_bounds(sr.double(), hr.double())
    _worst((out.cpu().double() - ref).abs(), torch.tensor([b_l1, b_tv], dtype=torch.double), f"{tag} [l1, tv]")
    unfused, fused = _l1_tv_grad_fp32(sr, hr, G_L1, G_TV)
    g64 = SO.l1_tv_grad(sr.double(), hr.double(), G_L1, G_TV)
    assert float((unfused.double() - g64).abs().max()) <= 2 * U * float(g64.abs().max())       # the fp32 evaluation is the oracle's, rounded
    eq_u, eq_f = torch.equal(grad.cpu(), unfused), torch.equal(grad.cpu(), fused)
    print(f"{tag} gradient: equal to the unfused fp32 evaluation {eq_u}, to the fused {eq_f}; "
          f"max |grad - float64| {float((grad.cpu().double() - g64).abs().max()):.3e}")
    assert eq_u or eq_f
    return out


def test_l1_tv_past_one_pass_against_float64():
    sr = detrand.image_batch((L1_N, L1_H, L1_W, 3), 51) + detrand.uniform((L1_N, L1_H, L1_W, 3), 52, -0.5, 0.5)
    hr = detrand.image_batch((L1_N, L1_H, L1_W, 3), 53)
    _check_l1_tv(sr, hr, "l1_tv random")


def test_l1_tv_with_equal_pixels_and_equal_neighbours():
    """sign(0) = 0: integer-valued images in 0 .. 3, a quarter of the differences are exactly zero."""
    sr, hr = SO.tied_images((L1_N, L1_H, L1_W, 3), 3)
    assert int((sr == hr).sum()) * 10 >= sr.numel()
    assert int((sr[:, :, :-1] == sr[:, :, 1:]).sum()) * 10 >= sr.numel() and int((sr[:, :-1] == sr[:, 1:]).sum()) * 10 >= sr.numel()
    _check_l1_tv(sr, hr, "l1_tv tied")


def test_tv_alone_through_l1_tv_of_an_image_with_itself():
    """functional.py's tv_loss: loss_l1_tv(sr, sr, 0, 1).  The L1 output is exactly 0 and the gradient is the integer count of signs."""
    from pesr_amd import ops
    sr = detrand.image_batch((L1_N, L1_H, L1_W, 3), 54) + detrand.uniform((L1_N, L1_H, L1_W, 3), 55, -0.5, 0.5)
    for need_grad in (True, False):
        out, grad = ops.loss_l1_tv(sr.cuda(), sr.cuda(), 0.0, 1.0, need_grad=need_grad)
        assert float(out[0]) == 0.0
        ref = SO.l1_tv_value(sr.double(), sr.double())
        _worst((out[1].cpu().double() - ref[1]).abs().reshape(1), torch.tensor([_l1_tv_sum_bounds(sr.double(), sr.double())[1]], dtype=torch.double), "tv alone")
        if need_grad:
            assert torch.equal(grad.cpu(), SO.tv_sign_count(sr))
        else:
            assert grad is None


# ================================================================================================
# MSE
# ================================================================================================
MSE_SHAPE = (2, 23, 23, 512)                                       # (2, 512, 23, 23) as NHWC: 541 696 floats, 135 424 float4


def test_mse_past_one_pass_against_float64():
    """Gradient: two roundings, the difference and its product with gscale.  Value, relative to the mean of the squares: a term is
    d^2 with d rounded (2 u) and squared (1), then 4 additions per pass (three inside a float4, one into the running sum) x passes, 6
    butterfly steps, 3 additions of the waves, and the fp32 store."""
    from pesr_amd import ops
    a, b = detrand.uniform(MSE_SHAPE, 1), detrand.uniform(MSE_SHAPE, 2)
    gscale = _f32(50 * 2.0 / a.numel())
    passes = _passes(a.numel() // 4, 512 * 256)
    assert passes == 2
    out, grad = ops.loss_mse(a.cuda(), b.cuda(), gscale)
    out2, none = ops.loss_mse(a.cuda(), b.cuda(), gscale, need_grad=False)
    assert none is None and torch.equal(out, out2)
    ref = SO.mse_value(a.double(), b.double())
    _worst((out.cpu().double() - ref).abs(), ((_k(3 + passes * 4 + 6 + 3 + 1) + D) * ref).reshape(1), "mse value")
    gref = SO.mse_grad(a.double(), b.double(), gscale)
    _worst((grad.cpu().double() - gref).abs(), _k(2) * gref.abs(), "mse gradient")
    out, grad = ops.loss_mse(a.cuda(), a.cuda(), gscale)
    assert float(out[0]) == 0.0 and float(grad.abs().max()) == 0.0


# ================================================================================================
# MeanShift
# ================================================================================================
def _meanshift_params():
    w = torch.eye(3) + detrand.uniform((3, 3), 2, -0.1, 0.1)
    return w.view(3, 3, 1, 1).contiguous(), detrand.uniform((3,), 3, -100, 100)


def _images(shape, seed):
    """Integers 0 .. 255 as fp32, [N, H, W, 3]."""
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("x_nchw", [False, True])
@pytest.mark.parametrize("y_nchw", [False, True])
def test_meanshift_forward_past_one_pass_all_layouts(x_nchw, y_nchw):
    """y_i = fma(w_i2, x_2, fma(w_i1, x_1, fma(w_i0, x_0, b_i))): three roundings, each of a partial sum that is at most |b_i| + sum_j
    |w_ij| |x_j|.  The 1e-6 of the largest output that test_meanshift asks stays the ceiling."""
    from pesr_amd import ops
    x = _images((2, 725, 725, 3), 1)
    w, b = _meanshift_params()
    xin = x.permute(0, 3, 1, 2).contiguous() if x_nchw else x
    y = ops.meanshift_fwd(xin.cuda(), w.cuda(), b.cuda(), x_nchw=x_nchw, y_nchw=y_nchw).cpu()
    y = y.permute(0, 2, 3, 1) if y_nchw else y
    ref = SO.meanshift_fwd(x.double(), w.double(), b.double())
    mag = SO.meanshift_fwd(x.double(), w.double().abs(), b.double().abs())
    err = (y.double() - ref).abs()
    _worst(err, _k(3) * mag, f"meanshift fwd x_nchw={x_nchw} y_nchw={y_nchw}")
    assert float(err.max()) <= 1e-6 * float(ref.abs().max())


@pytest.mark.parametrize("x_nchw", [False, True])
@pytest.mark.parametrize("need_dx", [True, False])
def test_meanshift_backward_past_one_pass_cancelling_sums(x_nchw, need_dx):
    """x an image batch in 0 .. 255, dy zero-mean: dw = sum dy x is a sum of large terms that mostly cancel, what the kernel's double
    accumulators are for.  dx: three roundings of partial sums <= sum_i |w_ij| |dy_i|.  dw, with A = sum |dy_i x_j|: the fp32 products
    (u A), every block's double partial sum rounded to fp32 (u |partial| each, in all <= u (1 + u) A), the double sum of the 1024
    partials, and the fp32 store (u |dw|):  |d dw| <= (2 u + 2 u^2 + D) A + u |dw|.  db has no products: (u + u^2 + D) sum |dy_i| + u |db|."""
    from pesr_amd import ops
    x = _images((L1_N, L1_H, L1_W, 3), 4)
    dy = detrand.uniform((L1_N, L1_H, L1_W, 3), 5)
    w, _ = _meanshift_params()
    xin = x.permute(0, 3, 1, 2).contiguous() if x_nchw else x
    dx, dw, db = ops.meanshift_bwd(dy.cuda(), xin.cuda(), w.cuda(), x_nchw=x_nchw, need_dx=need_dx)
    dx_ref, dw_ref, db_ref = SO.meanshift_bwd(dy.double(), x.double(), w.double())
    _, A, S = SO.meanshift_bwd(dy.double().abs(), x.double(), w.double().abs())
    tag = f"meanshift bwd x_nchw={x_nchw} need_dx={need_dx}"
    print(f"{tag}: sum |dy x| / |dw| = {float((A / dw_ref.abs()).min()):.0f} .. {float((A / dw_ref.abs()).max()):.0f}")
    _worst((dw.cpu().view(3, 3).double() - dw_ref).abs(), (2 * U + 2 * U * U + D) * A + U * dw_ref.abs(), f"{tag} dw")
    _worst((db.cpu().double() - db_ref).abs(), (U + U * U + D) * S + U * db_ref.abs(), f"{tag} db")
    if need_dx:
        _worst((dx.cpu().double() - dx_ref).abs(), _k(3) * (dy.double().abs() @ w.double().abs().reshape(3, 3)), f"{tag} dx")
    else:
        assert dx is None


# ================================================================================================
# 2x2 max-pool
# ================================================================================================
def test_maxpool_past_one_pass_is_pure_selection():
    from pesr_amd import ops
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(1, 2050, 2050, 8, generator=gen) * 2 - 1
    dy = torch.randn(1, 1025, 1025, 8, generator=gen)
    xg, dyg = x.cuda(), dy.cuda()
    assert torch.equal(ops.maxpool2x2_fwd(xg).cpu().permute(0, 3, 1, 2), F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2))
    for relu_in in (True, False):
        assert torch.equal(ops.maxpool2x2_bwd(xg, dyg, relu_in=relu_in).cpu(), SO.maxpool_bwd(x, dy, relu_in)), relu_in


@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (1, 3, 2, 4)])
def test_maxpool_forward_floor_mode_on_odd_sides(shape):
    from pesr_amd import ops
    x = detrand.uniform(shape, 1)
    y = ops.maxpool2x2_fwd(x.cuda()).cpu()
    assert y.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    assert torch.equal(y.permute(0, 3, 1, 2), F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2))


@pytest.mark.parametrize("relu_in", [True, False])
@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 14, 14, 64)])
def test_maxpool_backward_at_ties_takes_the_first_maximum(shape, relu_in):
    """Draws from {-1, 0, 1, 2} and one -0.0: VGG activations after a ReLU are full of equal zeros."""
    from pesr_amd import ops
    x = SO.tied_pool_input(shape, 5)
    tied, windows = SO.maxpool_tied_windows(x)
    assert 3 * tied >= windows, (tied, windows)
    dy = torch.randn(shape[0], shape[1] // 2, shape[2] // 2, shape[3], generator=torch.Generator().manual_seed(6))
    assert torch.equal(ops.maxpool2x2_fwd(x.cuda()).cpu(), SO.maxpool_fwd(x))
    assert torch.equal(ops.maxpool2x2_bwd(x.cuda(), dy.cuda(), relu_in=relu_in).cpu(), SO.maxpool_bwd(x, dy, relu_in))


# ================================================================================================
# relu_mask
# ================================================================================================
RELU_N = 4 * ((1 << 21) + 300)
# (reference, add, alpha, slope): the call shapes of functional.py - ReLU and LeakyReLU backward, the scaled add, the plain scale, the
# LeakyReLU forward with the input as its own reference - and the masked scaled add of test_maxpool_and_relu_mask with and without a slope
RELU_CASES = [("ref", False, 1.0, 0.0), ("ref", False, 1.0, 0.2), (None, True, 0.5, 0.0), (None, False, 0.5, 0.0), ("alias", False, 1.0, 0.2),
              ("ref", True, 0.5, 0.0), ("ref", True, 1.0, 0.2), ("ref", False, 0.5, 0.2)]
_relu_data = {}


def _relu_inputs():
    if not _relu_data:
        gen = torch.Generator().manual_seed(12)
        g, ref, add = (torch.randn(RELU_N, generator=gen) for _ in range(3))
        at = torch.arange(RELU_N)
        ref[at % 16 == 3] = 0.0                                     # an eighth of the positions: exact zeros of both signs
        ref[at % 16 == 11] = -0.0
        _relu_data.update(g=g, ref=ref, add=add)
    return _relu_data["g"], _relu_data["ref"], _relu_data["add"]


@pytest.mark.parametrize("ref_kind,with_add,alpha,slope", RELU_CASES)
def test_relu_mask_past_one_pass_with_zeros_of_both_signs(ref_kind, with_add, alpha, slope):
    """Against the fp32 evaluation of the oracle's expression: exact without an addend.  With one the compiler may fuse the last product
    with the sum, which then skips the product's rounding: at most one ulp, taken at the larger of the product and the result (under
    cancellation the result's own ulp is smaller than the rounding that the fused form does not make)."""
    from pesr_amd import ops
    g, ref, add = _relu_inputs()
    if ref_kind == "alias":
        g = ref
    r = None if ref_kind is None else ref
    assert r is None or (int((r == 0).sum()) * 20 >= RELU_N and bool(torch.signbit(r[r == 0]).any()) and not bool(torch.signbit(r[r == 0]).all()))
    gg = g.cuda()
    rg = None if r is None else (gg if ref_kind == "alias" else r.cuda())
    out = ops.relu_mask(gg, rg, add.cuda() if with_add else None, alpha=alpha, slope=slope).cpu()
    want = SO.relu_mask(g, r, add if with_add else None, alpha, slope)
    assert want.dtype == torch.float32
    if not with_add:
        assert torch.equal(out, want)
        return
    prod = SO.relu_mask(g, r, None, alpha, slope)
    _worst((out.double() - want.double()).abs(), _ulp(torch.maximum(prod.abs(), want.abs())), f"relu_mask {ref_kind} add alpha={alpha} slope={slope}")


# ================================================================================================
# PixelShuffle, PSNR-Y
# ================================================================================================
def test_pixel_shuffle_past_one_pass_odd_sides():
    from pesr_amd import ops
    x = torch.arange(16 * 363 * 365, dtype=torch.float32).reshape(1, 16, 363, 365)           # 2 119 920 scalars, all exact in fp32
    y = ops.pixel_shuffle_fwd(x.permute(0, 2, 3, 1).contiguous().cuda())
    assert torch.equal(y.cpu().permute(0, 3, 1, 2), O.pixel_shuffle(x))
    gy = torch.arange(x.numel(), dtype=torch.float32).reshape(1, 4, 726, 730) * 0.5
    gx = ops.pixel_shuffle_bwd(gy.permute(0, 2, 3, 1).contiguous().cuda())
    assert torch.equal(gx.cpu().permute(0, 3, 1, 2), O.pixel_unshuffle(gy))


def test_psnr_y_past_one_pass_with_clipped_values_and_halves():
    """257 x 256 pixels; values below 0 and above 255 (clipped) and values at exactly x.5 (rounded half to even, as numpy does).  Every
    term of the sum is an integer-valued double, so the sum is exact in any order: == with the host computation."""
    from oracle import image as OI
    from pesr_amd import ops
    H, W = 257, 256
    a = detrand.image_batch((1, 3, H, W), 41)
    b = a + detrand.uniform((1, 3, H, W), 42, -30, 30)
    a.view(-1)[3::13] += 0.5
    b.view(-1)[::7] = a.view(-1)[::7].floor() + 2.5
    b.view(-1)[5::29] = a.view(-1)[5::29].floor() - 1.5
    assert float(b.min()) < 0 and float(b.max()) > 255 and float(a.max()) > 255
    ref = OI.psnr_y(a, b)
    yo, yl = (OI.rgb2y(OI.tensor_to_img(t)).clip(0, 255).round() for t in (a, b))
    total = float(((yo - yl) ** 2).sum())                          # integers: exact
    for a_cl in (False, True):
        for b_cl in (False, True):
            ag = a.cuda().contiguous(memory_format=torch.channels_last) if a_cl else a.cuda()
            bg = b.cuda().contiguous(memory_format=torch.channels_last) if b_cl else b.cuda()
            out = ops.psnr_y(ag, bg).cpu()
            assert float(out[0]) == total * (1.0 / (H * W)), (a_cl, b_cl)          # the exact sum times the rounded 1 / pixels
            assert float(out[1]) == ref, (a_cl, b_cl, float(out[1]), ref)


# ================================================================================================
# GAN loss
# ================================================================================================
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000, 1024])
@pytest.mark.parametrize("gan_type,side,focal,gamma", SO.GAN_CASES)
def test_gan_loss_over_all_sixteen_waves(B, gan_type, side, focal, gamma):
    """One block of 16 waves, 1 <= B <= 1024: B = 63, 64, 65 straddle the first wave, 1000 leaves the last one partly filled.  Saturated
    logits sit in the first and in the last wave.  Reference: the oracle under autograd in float64.  Tolerance: the larger of what
    test_gan_loss_kernel_vs_oracle allows (2e-6 of the value, 5e-6 of the largest gradient) and four times the error of the oracle's own
    fp32 CPU evaluation against its float64 one on the same inputs - never anything measured from the kernel."""
    from pesr_amd import ops
    r, f = SO.gan_logits(B)
    v64, dr64, df64 = SO.gan_loss_and_grads(r.double(), f.double(), gan_type, side, focal, gamma, 0.7)
    v32, dr32, df32 = SO.gan_loss_and_grads(r, f, gan_type, side, focal, gamma, 0.7)
    rg, fg = r.cuda(), f.cuda()
    out, d_r, d_f = ops.gan_loss(rg, fg, gan_type, side, focal, gamma, 0.7)
    tol_fixed, tol_fp32 = 2e-6 * abs(float(v64)) + 1e-9, 4 * abs(float(v32) - float(v64))
    err = abs(float(out[0]) - float(v64))
    print(f"gan_loss B {B} {gan_type} side {side} focal {focal} gamma {gamma}: value error {err:.3e}, tolerance max({tol_fixed:.3e}, {tol_fp32:.3e})")
    assert err <= max(tol_fixed, tol_fp32)
    for name, got, g64, g32 in (("d_real", d_r, dr64, dr32), ("d_fake", d_f, df64, df32)):
        assert got.shape == g64.shape
        if float(g64.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, name
            continue
        tol_fixed, tol_fp32 = 5e-6 * float(g64.abs().max()), 4 * float((g32.double() - g64).abs().max())
        err = float((got.cpu().double() - g64).abs().max())
        print(f"    {name}: error {err:.3e}, tolerance max({tol_fixed:.3e}, {tol_fp32:.3e})")
        assert err <= max(tol_fixed, tol_fp32), name
    out_r, only_r, none = ops.gan_loss(rg, fg, gan_type, side, focal, gamma, 0.7, need_fake=False)
    assert none is None and torch.equal(only_r, d_r) and torch.equal(out_r, out)
    out_f, none, only_f = ops.gan_loss(rg, fg, gan_type, side, focal, gamma, 0.7, need_real=False)
    assert none is None and torch.equal(only_f, d_f) and torch.equal(out_f, out)


# ================================================================================================
# refusals
# ================================================================================================
def test_invalid_arguments_are_refused_and_touch_nothing():
    """PESR_EINVAL (-1) and PESR_EWORKSPACE (-2) come back before anything is launched.  Every buffer is large enough for the size
    rounded up, so a missing check would compute something, not read or write out of bounds."""
    from pesr_amd import _lib, ops
    L = _lib.lib()
    s, P = ops._stream(), ops._p
    gen = torch.Generator().manual_seed(21)
    new = lambda *shape: torch.randn(*shape, generator=gen).cuda()              # noqa: E731
    a, b, c, d = new(8), new(8), new(8), new(8)
    st = torch.zeros(6, device="cuda"); st[0] = LR
    x, dy, dx = new(1, 4, 4, 8), new(1, 2, 2, 8), new(1, 4, 4, 8)
    r, f, out1, d_r, d_f = new(1028), new(1028), new(1), new(1028), new(1028)
    img, img2, grad, out2 = new(1, 4, 4, 3), new(1, 4, 4, 3), new(1, 4, 4, 3), new(2)
    w9, dw, db = new(9), new(9), new(3)
    outd = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((65536,), 5, dtype=torch.uint8, device="cuda")
    every = (a, b, c, d, st, x, dy, dx, r, f, out1, d_r, d_f, img, img2, grad, out2, w9, dw, db, outd, ws)
    keep = [t.clone() for t in every]
    EINVAL, EWS = -1, -2
    for n in (5, 6, 7):
        assert L.pesr_relu_mask(P(a), P(b), P(c), P(d), n, 1.0, 0.0, s) == EINVAL
        assert L.pesr_mse_fwd_bwd(P(a), P(b), P(c), P(out1), n, 1.0, P(ws), ws.numel(), s) == EINVAL
        assert L.pesr_adam_step(P(a), P(b), P(c), P(d), n, LR, B1, B2, EPS, 1, 1.0, s) == EINVAL
        assert L.pesr_adam_step_dev(P(a), P(b), P(c), P(d), n, P(st), B1, B2, EPS, 1.0, s) == EINVAL
    for step in (0, -1):
        assert L.pesr_adam_step(P(a), P(b), P(c), P(d), 8, LR, B1, B2, EPS, step, 1.0, s) == EINVAL
    assert L.pesr_adam_step_dev(P(a), P(b), P(c), P(d), 8, None, B1, B2, EPS, 1.0, s) == EINVAL
    for B, gan, side in ((0, 0, 0), (1025, 0, 0), (-1, 2, 1), (16, 3, 0), (16, -1, 0), (16, 0, 2), (16, 0, -1)):
        assert L.pesr_gan_loss_fwd_bwd(P(r), P(f), B, gan, side, 0, 1.0, 1.0, P(out1), P(d_r), P(d_f), s) == EINVAL, (B, gan, side)
    for H, W, C in ((3, 4, 8), (4, 3, 8), (4, 4, 6), (4, 4, 2)):
        assert L.pesr_maxpool2x2_bwd(P(x), P(dy), P(dx), 1, H, W, C, 1, s) == EINVAL, (H, W, C)
    need = {"l1_tv": 64 + 1024 * 2 * 4, "mse": 64 + 512 * 4, "meanshift_bwd": 128 + 1024 * 12 * 4, "psnr_y": 256 * 8}
    calls = {
        "l1_tv": lambda nbytes: L.pesr_loss_l1_tv_fwd_bwd(P(img), P(img2), P(grad), P(out2), 1, 4, 4, 1.0, 1.0, P(ws), nbytes, s),
        "mse": lambda nbytes: L.pesr_mse_fwd_bwd(P(a), P(b), P(c), P(out1), 8, 1.0, P(ws), nbytes, s),
        "meanshift_bwd": lambda nbytes: L.pesr_meanshift_bwd(P(img), P(img2), P(w9), P(grad), P(dw), P(db), 1, 4, 4, 0, P(ws), nbytes, s),
        "psnr_y": lambda nbytes: L.pesr_psnr_y(P(img), P(img2), P(outd), 4, 4, 1, 1, P(ws), nbytes, s),
    }
    for name, call in calls.items():
        assert call(need[name] - 1) == EWS, name                   # one byte short
        assert call(0) == EWS, name
    torch.cuda.synchronize()
    for t, k in zip(every, keep):
        assert torch.equal(t, k)
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.adam_step(a, b, c, d, LR, B1, B2, EPS, 0)
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.relu_mask(new(6))
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.loss_mse(new(6), new(6), 1.0)
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.maxpool2x2_bwd(new(1, 4, 4, 6), new(1, 2, 2, 6), relu_in=True)
    # the same calls with exactly the bytes they need, and with valid arguments, run
    for name, call in calls.items():
        assert call(need[name]) == 0, name
    assert L.pesr_adam_step(P(a), P(b), P(c), P(d), 8, LR, B1, B2, EPS, 1, 1.0, s) == 0
    assert L.pesr_maxpool2x2_bwd(P(x), P(dy), P(dx), 1, 4, 4, 8, 1, s) == 0
    torch.cuda.synchronize()
    assert not torch.equal(a, keep[0]) and not torch.equal(dx, keep[7]) and not torch.equal(out2, keep[16]) and not torch.equal(outd, keep[20])
