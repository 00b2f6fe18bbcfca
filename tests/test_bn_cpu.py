"""CPU: tests/bn_oracle.py itself against F.batch_norm + F.leaky_relu and torch autograd in float64, first and second order, on inputs
small enough to read.  This is where the semantics tests/test_bn_gpu.py holds bn.hip to are pinned to ATen: the biased variance normalises,
the unbiased one goes into running_var (M = 1, where torch refuses, is the oracle's own definition), "not > 0 takes the slope" at 0.0 and
at -0.0, and gamma = 0.  The last test shows, with the oracle alone, that the ill-conditioned inputs of the GPU tests keep the share of
elements whose sign of z fp32 and float64 may disagree on under its cap."""
import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import bn_oracle as BO

EPS = 1e-5


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _inputs(shape, seed, positive_gamma=True):
    x = BC.randn(shape, seed).double() * 1.5 + 0.7
    C = shape[3]
    gamma = BC.randn((C,), seed + 1).double()
    if positive_gamma:
        gamma = gamma.abs() + 0.5
    return x, gamma, BC.randn((C,), seed + 2).double() * 0.3, BC.randn(shape, seed + 3).double()


def _aten_act(z, slope):
    return z if slope == 1.0 else F.leaky_relu(z, slope)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * (1.0 + float(b.abs().max())), err


@pytest.mark.parametrize("momentum", [0.1, 0.3])
@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_training_forward_and_running_statistics_are_atens(slope, momentum):
    x, gamma, beta, _ = _inputs((2, 3, 5, 4), 1)
    rm = BC.randn((4,), 7).double(); rv = BC.randn((4,), 8).double().abs() + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    bn = torch.nn.BatchNorm2d(4, eps=EPS, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    nb = 0
    for call in range(2):                                            # two calls in a row: the update feeds on its own output
        ref = _aten_act(bn(_nchw(x) + call), slope).detach()
        y, mean, var, invstd = BO.train_forward(x + call, gamma, beta, EPS, slope, y_nchw=True)
        rm, rv, nb = BO.running_update(rm, rv, nb, mean, var, BO.rows(x), momentum)
        _close(y, ref)
        _close(BO.apply(x + call, gamma, beta, mean, invstd, slope), ref.permute(0, 2, 3, 1))
        _close(rm, bn.running_mean); _close(rv, bn.running_var)
        assert nb == int(bn.num_batches_tracked) == call + 1
    # the biased variance normalises, the unbiased one is stored
    _close(var, x.add(1).var(BO.ROWS, unbiased=False))
    assert not torch.allclose(rv, (1 - momentum) * rv_t + momentum * var)


def test_one_row_is_the_oracles_own_definition():
    x, gamma, beta, _ = _inputs((1, 1, 1, 4), 2)
    with pytest.raises(ValueError):
        F.batch_norm(_nchw(x), None, None, gamma, beta, True, 0.1, EPS)
    y, mean, var, invstd = BO.train_forward(x, gamma, beta, EPS, 0.2)
    assert torch.equal(mean, x[0, 0, 0]) and torch.equal(var, torch.zeros(4, dtype=torch.float64))
    assert torch.equal(y[0, 0, 0], BO.act(beta, 0.2))               # xhat = 0
    rm, rv, nb = BO.running_update(torch.ones(4).double(), torch.full((4,), 2.0).double(), 5, mean, var, 1, 0.1)
    _close(rm, 0.9 + 0.1 * mean); _close(rv, torch.full((4,), 1.8, dtype=torch.float64)); assert nb == 6


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_backward_is_autograds(slope, training):
    x, gamma, beta, dy = _inputs((2, 4, 3, 4), 3, positive_gamma=False)          # negative gammas among them
    xr = _nchw(x).clone().requires_grad_(True); gr = gamma.clone().requires_grad_(True); br = beta.clone().requires_grad_(True)
    if training:
        mean, var, invstd = BO.batch_stats(x, EPS)
        rm = rv = None
    else:
        rm = BC.randn((4,), 9).double(); rv = BC.randn((4,), 10).double().abs() + 0.5
        mean, invstd = rm, 1.0 / torch.sqrt(rv + EPS)
    _aten_act(F.batch_norm(xr, rm, rv, gr, br, training, 0.1, EPS), slope).backward(_nchw(dy))
    dx, dgamma, dbeta = BO.backward(x, dy, gamma, beta, mean, invstd, slope, training)
    _close(_nchw(dx), xr.grad); _close(dgamma, gr.grad); _close(dbeta, br.grad)
    g0, b0 = BC.randn((4,), 12).double(), BC.randn((4,), 13).double()
    _, dg2, db2 = BO.backward(x, dy, gamma, beta, mean, invstd, slope, training, g0, b0)
    assert torch.equal(dg2, g0 + dgamma) and torch.equal(db2, b0 + dbeta)


def test_backward_of_the_backward_is_autograds_through_aten_and_through_the_first_order_formula():
    z, gamma, _, du = _inputs((2, 3, 4, 4), 4, positive_gamma=False)
    g = BC.randn(z.shape, 21).double() - 0.4
    mean, var, invstd = BO.batch_stats(z, EPS)
    want = BO.bwd_bwd(z, du, g, gamma, mean, invstd)
    # through ATen's double backward: dz = d(bn(z)) / dz applied to du
    zr = _nchw(z).clone().requires_grad_(True); gr = gamma.clone().requires_grad_(True); dr = _nchw(du).clone().requires_grad_(True)
    y = F.batch_norm(zr, None, None, gr, torch.zeros(4, dtype=torch.float64), True, 0.1, EPS)
    dz, = torch.autograd.grad(y, zr, dr, create_graph=True)
    l_du, l_z, l_ga = torch.autograd.grad((dz * _nchw(g)).sum(), (dr, zr, gr))
    _close(_nchw(want[0]), l_du); _close(_nchw(want[1]), l_z); _close(want[2], l_ga)
    # through the oracle's own first-order formula (statistics as functions of z)
    z2 = z.clone().requires_grad_(True); g2 = gamma.clone().requires_grad_(True); d2 = du.clone().requires_grad_(True)
    m2, _, s2 = BO.batch_stats(z2, EPS)
    dz2 = BO.backward_masked(BO.normalize(z2, m2, s2), d2, g2, s2)[0]
    got = torch.autograd.grad((dz2 * g).sum(), (d2, z2, g2))
    for a, b in zip(want, got):
        _close(a, b)


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_zero_of_either_sign_takes_the_slope(slope):
    z = torch.tensor([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324], dtype=torch.float64)
    dy = torch.tensor([3.0, 5.0, 7.0, 11.0, 13.0, 17.0], dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    yr = _aten_act(zr, slope)
    yr.backward(dy)
    y = BO.act(z, slope)
    assert torch.equal(y, yr.detach()) and torch.equal(torch.signbit(y), torch.signbit(yr.detach()))
    assert torch.equal(BO.act_grad(z, dy, slope), zr.grad)
    assert BO.act_grad(z, dy, slope)[:2].tolist() == [3.0 * slope, 5.0 * slope]


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_gamma_zero_beta_zero(slope):
    x, gamma, beta, dy = _inputs((2, 3, 3, 4), 5)
    gamma[1] = 0.0; beta[1] = 0.0; gamma[2] = 0.0
    mean, var, invstd = BO.batch_stats(x, EPS)
    xr = _nchw(x).clone().requires_grad_(True); gr = gamma.clone().requires_grad_(True); br = beta.clone().requires_grad_(True)
    _aten_act(F.batch_norm(xr, None, None, gr, br, True, 0.1, EPS), slope).backward(_nchw(dy))
    dx, dgamma, dbeta = BO.backward(x, dy, gamma, beta, mean, invstd, slope)
    _close(_nchw(dx), xr.grad); _close(dgamma, gr.grad); _close(dbeta, br.grad)
    assert not dx[..., 1].any() and not dx[..., 2].any()
    assert torch.equal(dbeta[1], (dy[..., 1] * slope).sum())         # every z of channel 1 is exactly 0: dz = slope * dy


def test_statistics_from_exact_partial_sums():
    x = torch.randint(-9, 10, (3, 4, 5, 4)).double()
    x[..., 2] = 7.0                                                   # constant: E[x^2] - mean^2 is exactly 0
    rows = x.reshape(6, 10, 4)
    part = torch.stack([rows.sum(1), (rows * rows).sum(1)], 1)        # [6][2][4]
    mean, var, invstd = BO.stats_from_part(part, 60, EPS)
    m0, v0, s0 = BO.batch_stats(x, EPS)
    _close(mean, m0); _close(var, v0); _close(invstd, s0)
    assert float(var[2]) == 0.0 and float(invstd[2]) == EPS ** -0.5
    part[0, 1, 3] -= 1e6                                              # sums that would give var < 0 are clamped
    assert float(BO.stats_from_part(part, 60, EPS)[1][3]) == 0.0
    dg, db = BO.sums_from_part(part, torch.ones(4).double(), torch.ones(4).double())
    assert torch.equal(db, 1 + part[:, 0].sum(0)) and torch.equal(dg, 1 + part[:, 1].sum(0))


def test_ill_conditioned_inputs_keep_the_ambiguous_share_under_its_cap():
    """The fp32 statistics a correct kernel hands over are the float64 ones rounded; with them the set A (|z| within the fp32 forward
    bound) of the conditioning input of tests/test_bn_gpu.py is counted per channel."""
    x = BC.conditioning_input().double()
    gamma, beta = (t.double() for t in BC.affine(8, 12))
    mean, var, invstd = BO.batch_stats(x, BC.EPS)
    A = BC.ambiguous(x, gamma, beta, mean.float().double(), invstd.float().double())
    share = A.double().mean(BO.ROWS)
    print("ambiguous share per channel:", share.tolist())
    assert float(share.max()) <= BC.AMBIGUOUS_CAP
    r = mean.abs() / var.sqrt()
    for c, nominal in zip(range(1, 6), (10, 30, 100, 255, 1000)):    # the sample's own r, within 5 % of the nominal one
        assert abs(float(r[c]) / nominal - 1.0) < 0.05
    assert float(var[6]) == 0.0 and float(var[7]) < BC.EPS
