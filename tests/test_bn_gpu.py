"""GPU: pesr_amd/csrc/bn.hip - BatchNorm2d + LeakyReLU forward, backward, eval backward and the backward of the backward - through
pesr_amd.ops against tests/bn_oracle.py in float64 (docs/experiments/bn_tests.md).  Every error is compared element by element or channel
by channel with a bound made of that element's / channel's own terms - never with a maximum over channels.

u = 2^-24 is one fp32 rounding, k of them in a row compound to (1 + u)^k - 1 (BC.k); a fused multiply-add rounds once where the count
assumes twice, so the bounds hold however the compiler contracts.  D = 2^-40 stands for the double-precision part of a sum (at most
rpb + nb <= 4624 additions at 2^-53).  The bounds:

  stand-alone statistics (bn_reduce_kernel<0> + bn_finalize_kernel, double up to the one fp32 store), dd = 2 (rpb + nb + 20) 2^-53:
      mean    u |mean| + dd mean|x|
      invstd  relative u + rho (1 + rho) / 2,  rho = dd (E[x^2] + mean^2) / (var + eps)      - 3e-8 at r = |mean| / std = 1000
  fused statistics (a conv epilogue adds n <= 18 values per thread in fp32, stores the row in fp32, double from there on):
      mean    u |mean| + k(n + 1) mean|z|
      invstd  relative u + rho (1 + rho) / 2,  rho = (k(n + 2) E[z^2] + 2 |mean| k(n + 1) mean|z|) / (var + eps)
              <= 3 k(n + 2) (1 + r^2) var / (var + eps): the factor r^2 STAYS - the epilogues' sums are fp32
  running statistics  u |new value| + momentum x (the double-precision part of the mean's / the variance's bound)
  y ("fed": the oracle gets the kernel's fp32 mean_invstd)   k(5) (|gamma xhat| + |beta|), times slope where z <= 0
  dbeta, dgamma       (k(2) + D) sum|dz|, (k(4) + D) sum|dz xhat|: the slope product, xhat's two roundings, the fp32 store
  dx                  |gamma s| [k(10) (|dz| + |mean dz| + |xhat mean(dz xhat)|) + (dbeta's bound + |xhat| dgamma's bound) / M];
                      eval: k(4) |gamma s dz|
  bn_bwd_bwd          see _check_bwd2: its five per-block partial sums are fp32, so the bound of Ga = mean(g du) - G1 m1 carries
                      u (mean|g du| + 2 mean|g| mean|du|) - the cancellation factor, stated, not removed

The kink: A is the set of elements with |z| within the fp32 forward bound (BC.ambiguous), where fp32 and float64 may disagree on z > 0.
y is held to 3 x the bound there, dx is compared outside A, the sums' bounds are widened by (1 - slope) sum_A |dy| (times |xhat| for
dgamma), and |A| <= 0.1 % of the elements is asserted in every case.

The float64 oracle is evaluated by torch on the device (the large cases hold 8.4 M elements); tests/test_bn_cpu.py pins the same
functions to ATen on the CPU.  Each check prints its worst error / bound before it asserts."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import bn_oracle as BO
from bn_cases import D, EPS, SLOPE, U, k
from oracle import detrand

pytestmark = pytest.mark.gpu

R = BO.ROWS


def _grid(M):
    """bn.hip's bn_grid: (rows per block, blocks) of the reduce kernels"""
    b = min(max(-(-M // 64), 1), 512)
    rpb = -(-M // b)
    return rpb, -(-M // rpb)


def test_the_sizes_reach_the_paths_they_are_chosen_for():
    assert _grid(65) == (33, 2) and _grid(7232) == (64, 113) and _grid(33075) == (65, 509) and _grid(1024) == (64, 16)
    assert _grid(2 * 725 * 725)[1] == 512 and _grid(2 * 257 * 256)[1] == 512
    per_pass = 8192 * 256                                            # float4 groups per pass of the apply kernels' grid-stride loop
    assert 2 * 725 * 725 * 2 > per_pass and 2 * 257 * 256 * 16 > per_pass
    assert (725 * 725 * 2) < per_pass < 2 * 725 * 725 * 2            # NCHW output: the image boundary falls inside the first pass


def _worst(err, bound, what):
    """max err / bound over float64 tensors, asserted <= 1; where the bound is 0 the error must be 0; a NaN fails."""
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    worst = math.inf if bool(torch.isnan(err).any()) else worst
    print(f"{what}: max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f}"
    return worst


def _dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _running(C, seed=None):
    """(running_mean, running_var, num_batches) on the device: the defaults, or a non-trivial start"""
    if seed is None:
        return torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros((), dtype=torch.long).cuda()
    return detrand.uniform((C,), seed, -2.0, 2.0).cuda(), detrand.uniform((C,), seed + 1, 0.5, 3.0).cuda(), torch.zeros((), dtype=torch.long).cuda()


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------
def _moments(x64):
    mean, var, invstd = BO.batch_stats(x64, EPS)
    return mean, var, invstd, x64.abs().mean(R), (x64 * x64).mean(R)


def _invstd_bound(invstd, var, b_var):
    rho = b_var / (var + EPS)
    return invstd * (U + 0.5 * rho * (1.0 + rho))


def _check_stats(stats, x64, b_mean_sum, b_var, what):
    """mean and invstd per channel; b_mean_sum, b_var: the bounds of the mean before its fp32 store and of the variance.
    -> the relative error of invstd per channel (the conditioning tables of the document)."""
    mean, var, invstd, _, _ = _moments(x64)
    _worst((stats[0].double() - mean).abs(), U * mean.abs() + b_mean_sum, what + " mean")
    e = (stats[1].double() - invstd).abs()
    _worst(e, _invstd_bound(invstd, var, b_var), what + " invstd")
    return e / invstd


def _standalone_bounds(x64):
    M = BO.rows(x64)
    rpb, nb = _grid(M)
    dd = 2.0 * (rpb + nb + 20) * 2.0 ** -53
    mean, _, _, absx, msq = _moments(x64)
    return dd * absx, dd * (msq + mean * mean)


def _fused_bounds(z64, n):
    mean, _, _, absx, msq = _moments(z64)
    return k(n + 1) * absx, k(n + 2) * msq + 2.0 * mean.abs() * k(n + 1) * absx


def _check_running(after, before, x64, b_mean_sum, b_var, momentum, what):
    """one update of (running_mean, running_var, num_batches) from `before` (fp32 clones taken in front of the call)"""
    M = BO.rows(x64)
    mean, var, _, _, _ = _moments(x64)
    mom = BC.f32(momentum)
    rm, rv, n = BO.running_update(before[0].double(), before[1].double(), int(before[2]), mean, var, M, mom)
    unb = M / (M - 1.0) if M > 1 else 1.0
    _worst((after[0].double() - rm).abs(), U * rm.abs() + mom * b_mean_sum + D * (before[0].double().abs() + mean.abs()), what + " running_mean")
    _worst((after[1].double() - rv).abs(), U * rv.abs() + mom * unb * b_var + D * (before[1].double().abs() + var), what + " running_var")
    assert int(after[2]) == n, what + " num_batches"


def _fed(x, gamma, beta, stats):
    x64, g64, b64, mean, invstd = x.double(), gamma.double(), beta.double(), stats[0].double(), stats[1].double()
    xh = BO.normalize(x64, mean, invstd)
    z = g64 * xh + b64
    A = BC.ambiguous(x64, g64, b64, mean, invstd)
    share = float(A.double().mean())
    assert share <= BC.AMBIGUOUS_CAP, f"ambiguous share {share:.2e} of the elements"
    return g64, b64, invstd, xh, z, A


def _check_y(y, x, gamma, beta, stats, slope, what, y_nchw=False):
    g64, b64, invstd, xh, z, A = _fed(x, gamma, beta, stats)
    s = BC.f32(slope)
    T = (g64 * xh).abs() + b64.abs()
    bound = torch.where(A, 3.0 * k(5) * T, k(5) * T * torch.where(z > 0, 1.0, s))
    yy = y.permute(0, 2, 3, 1) if y_nchw else y
    assert yy.shape == x.shape and y.is_contiguous()
    return _worst((yy.double() - BO.act(z, s)).abs(), bound, what + " y")


def _check_bwd(out, x, dy, gamma, beta, stats, slope, what, training=True):
    """dy NHWC.  out = (dx, dgamma or None, dbeta or None)"""
    g64, b64, invstd, xh, z, A = _fed(x, gamma, beta, stats)
    s = BC.f32(slope)
    M = BO.rows(x)
    dy64 = dy.double()
    dz = BO.act_grad(z, dy64, s)
    Bb = (k(2) + D) * dz.abs().sum(R) + (1.0 - s) * (dy64.abs() * A).sum(R)
    Bg = (k(4) + D) * (dz * xh).abs().sum(R) + (1.0 - s) * ((dy64 * xh).abs() * A).sum(R)
    dx, dgamma, dbeta = BO.backward_masked(xh, dz, g64, invstd, training)
    if out[1] is not None:
        _worst((out[1].double() - dgamma).abs(), Bg, what + " dgamma")
        _worst((out[2].double() - dbeta).abs(), Bb, what + " dbeta")
    gs = (g64 * invstd).abs()
    if training:
        bound = gs * (k(10) * (dz.abs() + (dbeta / M).abs() + (xh * (dgamma / M)).abs()) + Bb / M + xh.abs() * (Bg / M))
    else:
        bound = k(4) * gs * dz.abs()
    err = torch.where(A, 0.0, (out[0].double() - dx).abs())           # outside A only
    return _worst(err, bound, what + " dx")


def _check_bwd2(out, z, du, g, gamma, stats, what):
    """bn_bwd_bwd, fed the kernel's statistics.  Means of absolute values: A_d = mean|du|, A_g = mean|g|, A_dx = mean|du xhat|,
    A_gx = mean|g xhat|, A_gd = mean|g du|.  bn_bwd2_reduce_kernel rounds each block's five partial sums to fp32, so a mean's error is
    u x (the mean of its absolute terms), plus xhat's two roundings where xhat is a factor: d(m1) <= u A_d, d(G1) <= u A_g,
    d(m2) <= k(3) A_dx, d(Gx) <= k(3) A_gx, d(Ga) <= u (A_gd + 2 A_g A_d + |Ga|) - the last one carries the cancellation factor
    (A_gd / |Ga| is 50 .. 300 with du, g at channel means +3, -2).
      L_du    |gamma s| k(10) (|g| + A_g + |xhat| A_gx)                               chain: xhat 2, Gx 3, product, 2 differences, gamma s, product
      L_z     |gamma| s^2 [k(16) T + |xhat| d(Ga)],  T = |xhat| (|Ga| + 3 A_dx A_gx) + A_dx (|g| + A_g) + A_gx (|du| + A_d)
      L_gamma u |L_gamma| + s M [u (A_gd + 2 A_d A_g) + 2 k(3) A_dx A_gx] (1 + 2^-16)    (double from the reduced sums on)"""
    z64, du64, g64, ga64, mean, invstd = z.double(), du.double(), g.double(), gamma.double(), stats[0].double(), stats[1].double()
    M = BO.rows(z)
    xh, m1, m2, G1, Gx, Ga = BO.bwd_bwd_means(z64, du64, g64, mean, invstd)
    A_d, A_g, A_dx, A_gx, A_gd = du64.abs().mean(R), g64.abs().mean(R), (du64 * xh).abs().mean(R), (g64 * xh).abs().mean(R), (g64 * du64).abs().mean(R)
    l_du, l_z, l_ga = BO.bwd_bwd(z64, du64, g64, ga64, mean, invstd)
    gs = (ga64 * invstd).abs()
    worst = []
    if out[0] is not None:
        worst.append(_worst((out[0].double() - l_du).abs(), gs * k(10) * (g64.abs() + A_g + xh.abs() * A_gx), what + " L_du"))
    if out[1] is not None:
        dGa = (U + D) * (A_gd + 2.0 * A_g * A_d) + U * Ga.abs()
        T = xh.abs() * (Ga.abs() + 3.0 * A_dx * A_gx) + A_dx * (g64.abs() + A_g) + A_gx * (du64.abs() + A_d)
        worst.append(_worst((out[1].double() - l_z).abs(), gs * invstd * (k(16) * T + xh.abs() * dGa), what + " L_z"))
    if out[2] is not None:
        b = U * l_ga.abs() + invstd * M * (U * (A_gd + 2.0 * A_d * A_g) + 2.0 * k(3) * A_dx * A_gx) * (1.0 + 2.0 ** -16)
        worst.append(_worst((out[2].double() - l_ga).abs(), b, what + " L_gamma"))
    return worst


def _fwd(x, gamma, beta, run, momentum=0.1, slope=0.2, y_nchw=False, what="forward", check_running=True):
    """the stand-alone training forward with every check -> (y, stats, relative error of invstd per channel)"""
    from pesr_amd import ops
    before = [t.clone() for t in run]
    y, stats = ops.bn_lrelu_fwd(x, gamma, beta, *run, eps=1e-5, momentum=momentum, slope=slope, y_nchw=y_nchw)
    x64 = x.double()
    b_mean, b_var = _standalone_bounds(x64)
    rel = _check_stats(stats, x64, b_mean, b_var, what)
    if check_running:
        _check_running(run, before, x64, b_mean, b_var, momentum, what)
    _check_y(y, x, gamma, beta, stats, slope, what, y_nchw)
    return y, stats, rel


# ------------------------------------------------------------------------------------------------
# conditioning
# ------------------------------------------------------------------------------------------------
def test_conditioning_of_the_stand_alone_forward_and_backward():
    """r = |mean| / std from 0.35 to 1000, a constant channel and one whose variance is below eps: the statistics' bound does not
    depend on r.

    Measured on the MI355X: while bn_reduce_kernel rounded each block's partial sums to fp32, invstd missed the bound from r = 10 on -
    relative error 1.8e-7 at r = 10, 1.9e-6 at 30, 4.4e-5 at 100, 1.4e-4 at 255, 2.4e-4 at 1000 against u = 6.0e-8; worst error / bound
    2 617.  With the partials kept in double the errors are 5.8e-8, 2.6e-8, 3.9e-9, 1.5e-8, 7.9e-10 and the worst error / bound is 0.98.
    The same rounding made the stand-alone statistics of the cases with few blocks (M <= 65: geometry, ties, running statistics) miss
    their bounds by 1.01 .. 10.7 x, and by 309 241 x at M = 1 (docs/experiments/bn_tests.md)."""
    from pesr_amd import ops
    x, = _dev(BC.conditioning_input())
    gamma, beta = _dev(*BC.affine(8, 12))
    y, stats, rel = _fwd(x, gamma, beta, _running(8, seed=31), what="conditioning")
    print("invstd relative error per channel:", " ".join(f"{float(v):.2e}" for v in rel))
    # the constant channel: var = 0 exactly, xhat = 0, y = lrelu(beta) bit for bit
    c = 6
    assert float(stats[0, c]) == float(np.float32(1000.1))
    assert float(stats[1, c]) == float(np.float32(1.0 / math.sqrt(float(np.float32(1e-5)))))
    b = beta[c]
    assert torch.equal(y[..., c], torch.where(b > 0, b, b * SLOPE).expand(y.shape[:3]))
    dy, = _dev(BC.randn(x.shape, 13))
    _check_bwd(ops.bn_lrelu_bwd(x, dy, gamma, beta, stats), x, dy, gamma, beta, stats, 0.2, "conditioning")


def test_conditioning_of_the_backward_of_the_backward():
    """du and g at channel means +3 and -2: Ga = mean(g du) - G1 m1 cancels 6 against 6."""
    from pesr_amd import ops
    z, = _dev(BC.conditioning_input())
    gamma, beta = _dev(*BC.affine(8, 12))
    _, stats = ops.bn_lrelu_fwd(z, gamma, beta, None, None, None)
    du, g = _dev(BC.randn(z.shape, 14) + 3.0, BC.randn(z.shape, 15) - 2.0)
    _check_bwd2(ops.bn_bwd_bwd(z, du, g, gamma, stats), z, du, g, gamma, stats, "conditioning")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,kind", [(2, 37, 50, 64, 64, 2, "direct"), (16, 40, 44, 64, 64, 1, "wino4")])
def test_conditioning_of_the_statistics_a_conv_epilogue_leaves(N, H, W, Cin, Cout, stride, kind):
    """conv3x3_fwd_bn_stats with a bias that puts the channel means at r = 0.35 (none), 10 and 30.  A thread of the direct kernel adds at
    most 18 pixels of a channel (144-pixel tile x 64 float4 columns over 512 threads), a lane of the F(4,3) kernel its 18 outputs: n = 18.  The bound grows with r^2, and so
    does the error - the stand-alone pass on the same z is printed next to it."""
    from pesr_amd import ops
    x = detrand.uniform((N, Cin, H, W), 21, -1.0, 2.0); w = detrand.uniform((Cout, Cin, 3, 3), 22, -0.05, 0.05)
    bias = torch.tensor([0.0, 6.0, 18.0]).repeat(Cout)[:Cout].contiguous()
    gamma, beta = _dev(*BC.affine(Cout, 23))
    xg = _nhwc(x).cuda()
    wp = ops.pack_conv3x3_wino4(w.cuda(), 0) if kind == "wino4" else ops.pack_conv3x3(w.cuda(), 0)
    res = ops.conv3x3_fwd_bn_stats(xg, wp, bias.cuda(), Cout, stride)
    assert res is not None, "the planner refused a shape this test expects the fused kernel to cover"
    z, part = res
    zr = _nhwc(F.conv2d(x.double(), w.double(), bias.double(), stride, 1))
    assert float((z.cpu().double() - zr).abs().max()) <= 1e-5 * float(zr.abs().max()), "conv + bias"      # (tests/test_bn_fused_gpu.py's tolerance)
    run = _running(Cout, seed=33); before = [t.clone() for t in run]
    y, stats = ops.bn_finalize_apply(z, part, gamma, beta, *run)
    z64 = z.double()
    mean, var, _, _, _ = _moments(z64)
    r = mean.abs() / var.sqrt()
    print("r per bias group:", [round(float(r[i::3].mean()), 2) for i in range(3)])
    assert 0.1 < float(r[0::3].mean()) < 1.0 and 8.0 < float(r[1::3].mean()) < 12.0 and 25.0 < float(r[2::3].mean()) < 35.0
    b_mean, b_var = _fused_bounds(z64, 18)
    rel = _check_stats(stats, z64, b_mean, b_var, "fused")
    _check_running(run, before, z64, b_mean, b_var, 0.1, "fused")
    _check_y(y, z, gamma, beta, stats, 0.2, "fused")
    _, _, rel2 = _fwd(z, gamma, beta, _running(Cout), what="stand-alone on the same z")
    for i in range(3):
        print(f"invstd relative error, worst channel of bias group {i}: fused {float(rel[i::3].max()):.2e}, stand-alone {float(rel2[i::3].max()):.2e}")


def test_conditioning_of_the_statistics_the_rgb_conv_leaves():
    """conv_rgb_bn_lrelu_fwd on a 0..255 image with all-positive weights: r is about 8.  A thread adds the 256 / 16 = 16 pixels of its
    channels in its one tile (2 x 5 x 2 = 20 tiles, fewer than the grid's cap): n = 16."""
    from pesr_amd import ops
    N, H, W, C = 2, 37, 50, 64
    x = detrand.image_batch((N, H, W, 3), 41).cuda(); w = detrand.uniform((C, 3, 3, 3), 42, 0.0, 0.05).cuda()
    gamma, beta = _dev(*BC.affine(C, 43))
    run = _running(C, seed=35); before = [t.clone() for t in run]
    z, y, stats = ops.conv_rgb_bn_lrelu_fwd(x, w, gamma, beta, *run)
    z64 = z.double()
    mean, var, _, _, _ = _moments(z64)
    r = mean.abs() / var.sqrt()
    print(f"r: {float(r.min()):.2f} .. {float(r.max()):.2f}")
    assert 4.0 < float(r.min()) and float(r.max()) < 16.0
    b_mean, b_var = _fused_bounds(z64, 16)
    rel = _check_stats(stats, z64, b_mean, b_var, "rgb fused")
    print(f"invstd relative error, worst channel: {float(rel.max()):.2e}")
    _check_running(run, before, z64, b_mean, b_var, 0.1, "rgb fused")
    _check_y(y, z, gamma, beta, stats, 0.2, "rgb fused")


# ------------------------------------------------------------------------------------------------
# launch geometry of the reduce kernels
# ------------------------------------------------------------------------------------------------
# M = 1; M = 2 at C = 4 (256 row lanes, 2 rows); M = 65: 2 blocks of 33 and 32 rows, at every channel-lane shape - C = 12: 85 row lanes and
# one idle thread, 36: 28 row lanes and four idle, 1028 and 2048: a second trip of the channel-group loop (1028: with a single live lane);
# M = 7 232: 113 blocks, the first trip of bn_rows2's unrolled loop; 33 075: rpb = 65, 509 blocks - the cap of 512 reached, nb below it,
# the last block ragged (65 x 509 - 33 075 = 10 rows short)
GEOMETRY = [(1, 1, 1, 64), (1, 1, 2, 4), (1, 5, 13, 4), (1, 5, 13, 12), (1, 5, 13, 36), (1, 5, 13, 64), (1, 5, 13, 512), (1, 5, 13, 1028),
            (1, 5, 13, 2048), (1, 64, 113, 36), (1, 64, 113, 64), (3, 105, 105, 12), (3, 105, 105, 64)]


def _case(shape, seed, du_g=False):
    """x in mean 0.5, std 1.44 as the earlier tests have it (normal here), gamma, beta, dy; du_g: two more gradients"""
    C = shape[3]
    out = _dev(BC.randn(shape, seed) * 1.44 + 0.5, *BC.affine(C, seed + 1), BC.randn(shape, seed + 3))
    if du_g:
        out += _dev(BC.randn(shape, seed + 4) + 0.3, BC.randn(shape, seed + 5) - 0.2)
    return out


@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: "x".join(map(str, s)))
def test_launch_geometry_of_the_reduce_kernels(shape):
    from pesr_amd import ops
    C = shape[3]
    x, gamma, beta, dy, du, g = _case(shape, 50, du_g=True)
    y, stats, _ = _fwd(x, gamma, beta, _running(C, seed=37), what="geometry")
    _check_bwd(ops.bn_lrelu_bwd(x, dy, gamma, beta, stats), x, dy, gamma, beta, stats, 0.2, "geometry train")
    est = ops.bn_eval_stats(*_running(C, seed=39)[:2], 1e-5)
    _check_bwd(ops.bn_lrelu_eval_bwd(x, dy, gamma, beta, est), x, dy, gamma, beta, est, 0.2, "geometry eval", training=False)
    _check_bwd2(ops.bn_bwd_bwd(x, du, g, gamma, stats), x, du, g, gamma, stats, "geometry")


# ------------------------------------------------------------------------------------------------
# grid-stride loops past one pass (8192 blocks x 256 float4 groups = 2 097 152 per pass)
# ------------------------------------------------------------------------------------------------
BIG = [(2, 725, 725, 8), (2, 257, 256, 64)]          # 1 051 250 rows x 2 groups = 2 102 500; 131 584 rows x 16 = 2 105 344
_big = {}


def _big_case(shape):
    """inputs and the kernel's statistics of a large case, made once and left unchanged"""
    if shape not in _big:
        from pesr_amd import ops
        _big.clear()                                                  # one large case resident at a time
        x, gamma, beta, dy = _case(shape, 60)
        _, stats = ops.bn_lrelu_fwd(x, gamma, beta, None, None, None)
        _big[shape] = (x, gamma, beta, dy, stats)
    return _big[shape]


@pytest.mark.parametrize("y_nchw", [False, True], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_forward_past_one_pass(shape, y_nchw):
    x, gamma, beta, _, _ = _big_case(shape)
    _fwd(x, gamma, beta, _running(shape[3]), y_nchw=y_nchw, what="past one pass")


@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_backward_past_one_pass(shape):
    from pesr_amd import ops
    x, gamma, beta, dy, stats = _big_case(shape)
    _check_bwd(ops.bn_lrelu_bwd(x, dy, gamma, beta, stats), x, dy, gamma, beta, stats, 0.2, "past one pass, train")
    out = ops.bn_lrelu_eval_bwd(x, dy, gamma, beta, stats, need_param_grads=False)
    assert out[1] is None and out[2] is None
    _check_bwd(out, x, dy, gamma, beta, stats, 0.2, "past one pass, eval without parameter gradients", training=False)


@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_backward_of_the_backward_past_one_pass_with_each_output_switched_off(shape):
    from pesr_amd import ops
    z, gamma, _, du, stats = _big_case(shape)
    g, = _dev(BC.randn(shape, 66) - 0.2)
    full = ops.bn_bwd_bwd(z, du, g, gamma, stats)
    _check_bwd2(full, z, du, g, gamma, stats, "past one pass")
    for off in range(3):
        need = [i != off for i in range(3)]
        out = ops.bn_bwd_bwd(z, du, g, gamma, stats, *need)
        for i in range(3):
            assert (out[i] is None) if i == off else torch.equal(out[i], full[i]), (off, i)


@pytest.mark.parametrize("shape", [(2, 3, 11, 4), (3, 1, 1, 8), (2, 5, 7, 36)], ids=lambda s: "x".join(map(str, s)))
def test_gradient_arriving_nchw(shape):
    """The transposer's 32 x 32 tiles at HW = 33 (one pixel into a second tile) with C = 4, at HW = 1 (no copy: the layouts coincide),
    and at HW = 35, C = 36 (both tiles ragged)."""
    from pesr_amd import ops
    x, gamma, beta, dy = _case(shape, 70)
    dyc = dy.permute(0, 3, 1, 2).contiguous()
    _, stats = ops.bn_lrelu_fwd(x, gamma, beta, None, None, None)
    _check_bwd(ops.bn_lrelu_bwd(x, dyc, gamma, beta, stats, dy_nchw=True), x, dy, gamma, beta, stats, 0.2, "nchw train")
    _check_bwd(ops.bn_lrelu_eval_bwd(x, dyc, gamma, beta, stats, dy_nchw=True), x, dy, gamma, beta, stats, 0.2, "nchw eval", training=False)


# ------------------------------------------------------------------------------------------------
# the row reducers on sums every order of addition gives exactly
# ------------------------------------------------------------------------------------------------
ROWS = [1, 16, 17, 112, 113, 129, 512, 513, 960, 961, 2049]      # 512: the last bn_*_kernel<64>, 513: the first <16>; 113, 129 and 961: the
#                                                                   first rows of the eight-deep unrolled loop of either shape


def _integer_part(rows, C, seed):
    """part [rows][2][C] of integers: column 0 in [-2^20, 2^20] - pairs (v, -v) plus offsets in [-64, 64], so the total stays small and
    a variance >= 0 exists for M = 256 -, column 1 (the squares' sums) in [2^19, 2^20]."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randint(-(1 << 20) + 64, (1 << 20) - 63, (rows // 2, C), generator=gen)
    s = torch.cat([v, -v, torch.zeros(rows % 2, C, dtype=torch.long)])[torch.randperm(rows, generator=gen)]      # the pairs cancel
    s = s + torch.randint(-64, 65, (rows, C), generator=gen)
    ss = torch.randint(1 << 19, (1 << 20) + 1, (rows, C), generator=gen)
    return torch.stack([s, ss], 1)


def _ulps(a, b):
    """distance in fp32 units in the last place (finite values of one sign)"""
    return (a.cpu().contiguous().view(torch.int32).long() - b.cpu().contiguous().view(torch.int32).long()).abs()


@pytest.mark.parametrize("C", [4, 20, 64, 68])
def test_row_reducers_on_exact_integer_sums(C):
    from pesr_amd import ops
    M = 256
    z, gamma, beta, gm = _case((1, 2, 128, C), 80)
    for rows in ROWS:
        ip = _integer_part(rows, C, 81 + rows)
        assert int(ip[:, 0].abs().max()) <= 1 << 20 and int(ip[:, 1].min()) >= 0
        part = ip.float().cuda()
        assert torch.equal(part.cpu().long(), ip)
        p64 = ip.numpy().astype(np.float64)
        s, ss = p64[:, 0].sum(0), p64[:, 1].sum(0)
        assert np.array_equal(s, ip[:, 0].sum(0).numpy()) and np.array_equal(ss, ip[:, 1].sum(0).numpy())     # exact in float64
        mean = s / M
        var = ss / M - mean * mean
        assert (var >= 0).all()
        eps = float(np.float32(1e-5))
        run = _running(C, seed=83); before = [t.clone().cpu() for t in run]
        _, stats = ops.bn_finalize_apply(z, part, gamma, beta, *run)
        want = torch.from_numpy(np.stack([mean, 1.0 / np.sqrt(var + eps)]).astype(np.float32))
        assert int(_ulps(stats, want).max()) <= 1, f"rows {rows}: mean_invstd"
        mom = float(np.float32(0.1))
        rm = ((1.0 - mom) * before[0].numpy().astype(np.float64) + mom * mean).astype(np.float32)
        rv = ((1.0 - mom) * before[1].numpy().astype(np.float64) + mom * (var * M / (M - 1))).astype(np.float32)
        assert int(_ulps(run[0], torch.from_numpy(rm)).max()) <= 1 and int(_ulps(run[1], torch.from_numpy(rv)).max()) <= 1 and int(run[2]) == 1
        # backward: the same rows read as sums of g' and of g' xhat
        _, dg, db = ops.bn_lrelu_bwd_fused(z, gm, part, gamma, beta, stats)
        assert torch.equal(db.cpu(), torch.from_numpy(s.astype(np.float32))), f"rows {rows}: dbeta"
        assert torch.equal(dg.cpu(), torch.from_numpy(ss.astype(np.float32))), f"rows {rows}: dgamma"
        g0, b0 = (torch.randint(-1000, 1000, (C,), generator=torch.Generator().manual_seed(84 + i)).float() for i in range(2))
        dg2, db2 = g0.clone().cuda(), b0.clone().cuda()
        ops.bn_lrelu_bwd_fused(z, gm, part, gamma, beta, stats, dgamma_out=dg2, dbeta_out=db2, accumulate=True)
        assert torch.equal(db2.cpu(), b0 + db.cpu()) and torch.equal(dg2.cpu(), g0 + dg.cpu()), f"rows {rows}: accumulate"      # one fp32 addition
    # sums that are not consistent (fp32 epilogue sums need not be): mean 5, E[x^2] = 25 - (1 + c) / 256 -> var < 0 is clamped to 0
    ip = _integer_part(17, C, 85)
    ip[0, 0] += 5 * M - ip[:, 0].sum(0)
    ip[:, 1] = 0
    ip[3, 1] = 25 * M - 1 - torch.arange(C)
    run = _running(C, seed=83); before = [t.clone().cpu() for t in run]
    _, stats = ops.bn_finalize_apply(z, ip.float().cuda(), gamma, beta, *run)
    assert torch.equal(stats[0].cpu(), torch.full((C,), 5.0))
    assert torch.equal(stats[1].cpu(), torch.full((C,), float(np.float32(1.0 / math.sqrt(float(np.float32(1e-5)))))))
    rv = ((1.0 - float(np.float32(0.1))) * before[1].numpy().astype(np.float64)).astype(np.float32)
    assert int(_ulps(run[1], torch.from_numpy(rv)).max()) <= 1


# ------------------------------------------------------------------------------------------------
# running statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.1, 0.3])
def test_running_statistics_over_two_calls_from_a_non_trivial_start(momentum):
    from pesr_amd import ops
    x, gamma, beta, _ = _case((2, 9, 11, 8), 90)
    run = _running(8, seed=91)
    _fwd(x, gamma, beta, run, momentum=momentum, what="first call")
    y, stats, _ = _fwd(x + 1.0, gamma, beta, run, momentum=momentum, what="second call")
    assert int(run[2]) == 2
    # all three pointers null: the same y and statistics, nothing else written
    y2, stats2 = ops.bn_lrelu_fwd(x + 1.0, gamma, beta, None, None, None, momentum=momentum)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)


# ------------------------------------------------------------------------------------------------
# ties and signs
# ------------------------------------------------------------------------------------------------
def _tie_case():
    """[2, 9, 11, 8]: channel 0 has gamma = beta = 0 (every z is exactly 0); channel 1 gamma < 0; channels 2 and 3 hold 66 pixels each of
    3, 2 and 4 - the mean is 3 exactly, in fp32 too - with beta = 0, so 66 pixels have z = +0.0 exactly (3: with gamma < 0)."""
    x = BC.randn((2, 9, 11, 8), 95) * 1.44 + 0.5
    t = torch.tensor([3.0, 2.0, 4.0]).repeat_interleave(66)[torch.randperm(198, generator=torch.Generator().manual_seed(96))].reshape(2, 9, 11)
    x[..., 2] = t; x[..., 3] = t
    gamma, beta = BC.affine(8, 97)
    gamma[0] = 0.0; beta[0] = 0.0; gamma[1] = -gamma[1]; beta[2] = 0.0; beta[3] = 0.0; gamma[3] = -gamma[3]
    return x, gamma, beta, t == 3.0


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_ties_at_the_kink_zero_gamma_and_negative_gamma(slope):
    from pesr_amd import ops
    x, gamma, beta, at_mean = _tie_case()
    x, gamma, beta, dy = _dev(x, gamma, beta, BC.randn(x.shape, 98))
    y, stats, _ = _fwd(x, gamma, beta, _running(8), slope=slope, what="ties")
    assert float(stats[0, 2]) == 3.0 and float(stats[0, 3]) == 3.0
    assert not y[..., 0].any() and not y[..., 2][at_mean].any() and not y[..., 3][at_mean].any()
    out = ops.bn_lrelu_bwd(x, dy, gamma, beta, stats, slope=slope)
    _check_bwd(out, x, dy, gamma, beta, stats, slope, "ties train")
    assert not out[0][..., 0].any()                                   # gamma = 0: dx = 0
    # channel 0, every z = 0: dz = slope * dy, to the bound of a plain sum (z >= 0 for z > 0 would give sum(dy))
    s = BC.f32(slope)
    want = s * dy[..., 0].double().sum()
    assert abs(float(out[2][0]) - float(want)) <= (k(2) + D) * s * float(dy[..., 0].double().abs().sum())
    out = ops.bn_lrelu_eval_bwd(x, dy, gamma, beta, stats, slope=slope)
    _check_bwd(out, x, dy, gamma, beta, stats, slope, "ties eval", training=False)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(99)).cuda()
    _check_bwd2(ops.bn_bwd_bwd(x, dy, g, gamma, stats), x, dy, g, gamma, stats, "ties")
