"""GPU: the Adam kernels with the moving average of the parameters fused in (pesr_adam_ema_step / pesr_adam_ema_step_dev,
pesr_amd/csrc/adam.hip, docs/modes.md section 4i).

Sizes follow the launch geometry - 256 threads, a grid capped at 8192 blocks, so the two-float4-per-pass loop only runs above
8192 * 256 = 2 097 152 float4:
    4                  one float4
    4 * 257            a second, partial block
    4 * (2^21 + 1)     the first element to enter the two-per-pass loop, everything else in the tail
    4 * (5 * 2^20 + 3) two-per-pass, then a ragged tail (84 MB per buffer)

p, m, v must equal the plain entry point's bit for bit.  The average is held against a float64 evaluation of
e' = e + (p' - e) * (1 - d) fed the kernel's own fp32 p' sequence (Adam's error does not enter), with the bound
|e - e64| <= k * 2^-22 * max(|e|, |p|) after k steps: per step one rounding in the subtraction (2^-24 |p' - e|, scaled by
1 - d) and at most one and a half in the multiply-add (2^-24 |e'| when it is one fused operation), and the error already
there is carried on with the factor d < 1."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [4, 4 * 257, 4 * ((1 << 21) + 1), 4 * (5 * (1 << 20) + 3)]
LR, B1, B2, EPS, GSCALE = 5e-5, 0.9, 0.999, 1e-8, 0.5
STEPS = 3


def _buffers(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, device="cuda", generator=g)
    m = torch.randn(n, device="cuda", generator=g) * 1e-2
    v = torch.rand(n, device="cuda", generator=g) * 1e-3
    e = p + torch.randn(n, device="cuda", generator=g) * 0.1      # an average that lags its parameters
    grads = [torch.randn(n, device="cuda", generator=g) for _ in range(STEPS)]
    return p, m, v, e, grads


def _dev_state(lr):
    st = torch.zeros(6, device="cuda")
    st[0] = lr
    return st


@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-state"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_form_leaves_adam_bit_identical_and_the_average_within_fp32_rounding(n, dev):
    from pesr_amd import ops
    decay = 0.999 if dev else 0.9
    one_minus_d = float(np.float32(1.0) - np.float32(decay))           # formed once, in fp32, as the launcher does
    p, m, v, e, grads = _buffers(n, 7 + n % 1000)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    e64 = e.double()
    st, st2 = (_dev_state(LR), _dev_state(LR)) if dev else (None, None)
    for k in range(1, STEPS + 1):
        g = grads[k - 1]
        g_before = g.clone()
        if dev:
            ops.adam_ema_step_dev(p, g, m, v, e, decay, st, B1, B2, EPS, GSCALE)
            ops.adam_step_dev(p2, g, m2, v2, st2, B1, B2, EPS, GSCALE)
        else:
            ops.adam_ema_step(p, g, m, v, e, decay, LR, B1, B2, EPS, k, GSCALE)
            ops.adam_step(p2, g, m2, v2, LR, B1, B2, EPS, k, GSCALE)
        assert torch.equal(g, g_before)
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), (n, k)
        e64 = e64 + (p.double() - e64) * one_minus_d
        bound = k * 2.0 ** -22 * torch.maximum(e.abs(), p.abs()).double()
        err = (e.double() - e64).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"n {n} step {k}: max |e - e64| {float(err.max()):.3e}, worst error / bound {worst:.3f}")
        assert bool((err <= bound).all()), (n, k, worst)
    assert not torch.equal(e, p) and float((e - p).abs().max()) > 1e-3     # it is an average, not a copy
    if dev:
        assert torch.equal(st, st2) and st.view(torch.int32)[4].item() == STEPS


def test_the_average_moves_towards_the_parameters_by_one_minus_decay():
    """A value check that does not lean on the float64 recurrence: zero gradient and zero moments leave p where it is, and the
    average closes exactly the fraction 1 - d of its distance per step."""
    from pesr_amd import ops
    n = 4 * 300
    p = torch.full((n,), 2.0, device="cuda")
    e = torch.zeros(n, device="cuda")
    m, v, g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ops.adam_ema_step(p, g, m, v, e, 0.75, LR, B1, B2, EPS, 1)
    assert bool((p == 2.0).all()) and bool((e == 0.5).all())
    ops.adam_ema_step_dev(p, g, m, v, e, 0.75, _dev_state(LR), B1, B2, EPS)
    assert bool((p == 2.0).all()) and bool((e == 0.875).all())


def test_invalid_arguments_are_refused_and_touch_nothing():
    from pesr_amd import _lib, ops
    L = _lib.lib()
    n = 8
    p, m, v, e, grads = _buffers(n, 3)
    g = grads[0]
    st = _dev_state(LR)
    keep = [t.clone() for t in (p, g, m, v, e, st)]
    s = ops._stream()
    P = ops._p

    def host(n_=n, ema=e, decay=0.9, step=1):
        return L.pesr_adam_ema_step(P(p), P(g), P(m), P(v), n_, LR, B1, B2, EPS, step, 1.0, P(ema), decay, s)

    def devf(n_=n, ema=e, decay=0.9, state=st):
        return L.pesr_adam_ema_step_dev(P(p), P(g), P(m), P(v), n_, P(state), B1, B2, EPS, 1.0, P(ema), decay, s)

    for f in (host, devf):
        assert f(n_=6) == -1                              # n % 4 != 0
        assert f(ema=None) == -1                          # no average to update
        for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
            assert f(decay=bad) == -1, bad                # the decay lies inside (0, 1)
    assert host(step=0) == -1
    assert devf(state=None) == -1
    torch.cuda.synchronize()
    for t, k in zip((p, g, m, v, e, st), keep):
        assert torch.equal(t, k)                          # (the device-state form did not advance its count either)
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.adam_ema_step(p, g, m, v, e, 1.0, LR, B1, B2, EPS, 1)
    assert host() == 0 and devf() == 0                    # and the same calls with valid arguments run
    torch.cuda.synchronize()
    assert not torch.equal(p, keep[0]) and not torch.equal(e, keep[4]) and st.view(torch.int32)[4].item() == 1
