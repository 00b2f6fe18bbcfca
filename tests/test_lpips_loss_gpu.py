"""GPU: LPIPS as a training loss (docs/modes.md section 4o).

The head's gradient (pesr_amd/csrc/lpips.hip through ops.lpips_layer_bwd) against tests/lpips_grad_oracle.py grad_ordered BIT FOR BIT:
the kernel's order of operations is fixed and nothing is fused, so kernel and restatement perform the same IEEE operations, the one
rounding to float32 included.  How far grad_ordered is from the formula, and the formula from autograd on the definition, is bounded
on the CPU (tests/test_lpips_loss_cpu.py).  The rule at a pixel whose `a` vector is all zero - the gradient is 0 there, a definition,
where the formula gives 2 w t / 1e-10 and autograd NaN - is part of grad_ordered and so of every comparison here.

The two-pointer forward against the [a; b] forward, bit for bit.  lpips_loss against lpips(), bit for bit.  The whole gradient
d(sum of scores) / d(sr) against the float64 CPU trunk, allowed three times the error of the CPU's float32 trunk (the rule of
helpers.grads_vs_fp64), at image seeds chosen on the CPU (tests/lpips_trunk_grad.py says which and why), and the same bits with the
bf16 mode set around the backward.  Then the training step."""
import numpy as np
import pytest
import torch

import lpips_cases as C
import lpips_grad_cases as G
import lpips_trunk_grad as T
import loss_step_harness as HS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _check_bwd(c, n, h, w, kind):
    from pesr_amd import ops
    fa, fb, wt, g = G.case(c, n, h, w, kind)
    want = G.ordered(c, n, h, w, kind)
    da, db, dw, dg = _dev(fa), _dev(fb), _dev(wt), _dev(g)
    got = ops.lpips_layer_bwd(da, db, dw, dg)
    assert got.dtype == torch.float32 and got.shape == (n, h, w, c) and got.is_contiguous()
    assert torch.equal(ops.lpips_layer_bwd(da, db, dw, dg), got)                                  # the same bits on every call
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.argwhere(_bits(got) != _bits(want))
        pytest.fail(f"C {c} {n} x {h} x {w} {kind}: {len(bad)} of {want.size} elements differ, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}, max |diff| {np.max(np.abs(got.astype(np.float64) - want)):.3e}")
    return got, (fa, fb, wt, g)


# ---- the head's gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w", [(c, h, w) for c in G.CHANNELS for (h, w) in G.SHAPES])
def test_head_backward_bit_for_bit(c, h, w):
    for n in G.BATCHES:
        got, (_, _, _, g) = _check_bwd(c, n, h, w, "relu")
        assert np.abs(got).max() > 0 and (n == 1 or g[0] != g[1])     # distinct values of g per image


@pytest.mark.parametrize("c,n,h,w", G.SPECIAL)
def test_head_backward_special_cases_bit_for_bit(c, n, h, w):
    """An all-zero `a` pixel (the gradient is the DEFINED 0 there, not the formula's 2 w t / 1e-10 and not NaN), b == a (all zeros),
    b ~ a (t cancels), zero weight channels."""
    for kind in ("zeros", "same", "near", "wzeros"):
        got, (fa, fb, wt, g) = _check_bwd(c, n, h, w, kind)
        if kind == "zeros":
            dead = (fa == 0).all(-1)
            assert dead.any() and (fb[dead] > 0).any() and bool((got[dead] == 0).all())
        if kind == "same":
            assert bool((got == 0).all())
        if kind == "wzeros":
            assert bool((wt == 0).any())


def test_head_backward_margins_and_refusals():
    """Inputs surrounded by NaN (a read outside would poison the gradient), the output surrounded by a sentinel; then the refusals."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    M, sentinel = 4096, -12345.678
    for (c, n, h, w) in ((64, 2, 5, 13), (512, 2, 5, 13), (256, 1, 1, 17)):
        fa, fb, wt, g = G.case(c, n, h, w, "relu")
        want = G.ordered(c, n, h, w, "relu")
        flat = {}
        for name, arr in (("fa", fa), ("fb", fb), ("w", wt)):
            t = torch.full((arr.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
            t[M:M + arr.size] = _dev(arr).reshape(-1)
            flat[name] = t
        gd = torch.full((n + 2 * M,), float("nan"), dtype=torch.float64, device=DEV)
        gd[M:M + n] = _dev(g)
        out = torch.full((fa.size + 2 * M,), sentinel, dtype=torch.float32, device=DEV)
        args = lambda cc: (flat["fa"].data_ptr() + 4 * M, flat["fb"].data_ptr() + 4 * M, flat["w"].data_ptr() + 4 * M, gd.data_ptr() + 8 * M,
                           out.data_ptr() + 4 * M, n, h, w, cc, stream)
        assert lib.pesr_lpips_layer_bwd(*args(c)) == 0
        torch.cuda.synchronize()
        assert bool((out[:M] == np.float32(sentinel)).all()) and bool((out[M + fa.size:] == np.float32(sentinel)).all())
        assert np.array_equal(_bits(out[M:M + fa.size].reshape(fa.shape).cpu().numpy()), _bits(want))
        keep = out.clone()
        for bad_c in (96, 32, 1024):
            assert lib.pesr_lpips_layer_bwd(*args(bad_c)) == -1
        torch.cuda.synchronize()
        assert torch.equal(out, keep)
    a, wv, gv = torch.zeros(2, 3, 5, 64, device=DEV), torch.ones(64, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV)
    big = torch.zeros(2, 3, 5, 128, device=DEV)
    with pytest.raises(_lib.PesrHipError, match="contiguous"):
        ops.lpips_layer_bwd(big[:, :, :, :64], a, wv, gv)
    with pytest.raises(_lib.PesrHipError, match="contiguous"):
        ops.lpips_layer_pair(a, big[:, :, :, :64], wv)
    with pytest.raises(_lib.PesrHipError, match="one shape"):
        ops.lpips_layer_bwd(a, a[:1], wv, gv)
    with pytest.raises(_lib.PesrHipError, match="weights"):
        ops.lpips_layer_bwd(a, a, torch.ones(128, device=DEV), gv)
    with pytest.raises(_lib.PesrHipError, match="float64"):
        ops.lpips_layer_bwd(a, a, wv, gv.float())
    with pytest.raises(_lib.PesrHipError, match="float64"):
        ops.lpips_layer_bwd(a, a, wv, gv[:1])
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.lpips_layer_bwd(torch.zeros(2, 3, 5, 96, device=DEV), torch.zeros(2, 3, 5, 96, device=DEV), torch.ones(96, device=DEV), gv)
    with pytest.raises(_lib.PesrHipError):
        ops.lpips_layer_bwd(a.cpu(), a.cpu(), wv.cpu(), gv.cpu())


# ---- the forward with two pointers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.CHANNELS)
def test_two_pointer_forward_equals_the_concatenated_one(c):
    from pesr_amd import ops
    for (h, w) in G.SHAPES:
        for n in G.BATCHES:
            for kind in ("relu", "zeros") if (h, w) == (5, 13) else ("relu",):
                fa, fb, wt, _ = G.case(c, n, h, w, kind)
                # fb in an allocation of its own, not behind fa
                da, spacer, db, dw = _dev(fa), torch.empty(1031, device=DEV), _dev(fb), _dev(wt)
                score, dmap = ops.lpips_layer_pair(da, db, dw, return_map=True)
                want_score, want_map = ops.lpips_layer(torch.cat([da, db]), dw, return_map=True)
                assert score.dtype == torch.float64 and score.shape == (n,) and dmap.shape == (n, h, w)
                assert torch.equal(score, want_score) and torch.equal(dmap, want_map), (c, n, h, w, kind)
                assert torch.equal(ops.lpips_layer_pair(da, db, dw), score)
                del spacer


def test_layer_function_gives_a_gradient_to_fa_only():
    from pesr_amd import functional as PF
    fa, fb, wt, g = G.case(128, 2, 5, 13, "relu")
    da, db, dw = _dev(fa).requires_grad_(), _dev(fb).requires_grad_(), _dev(wt).requires_grad_()
    score = PF.lpips_layer(da, db, dw)
    assert score.dtype == torch.float64 and score.shape == (2,)
    (score * _dev(g)).sum().backward()
    assert db.grad is None and dw.grad is None
    assert np.array_equal(_bits(da.grad.cpu().numpy()), _bits(G.ordered(128, 2, 5, 13, "relu")))


# ---- the metric is unchanged, and the loss is the metric ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shave", [(s, v) for (s, v) in C.METRIC_CASES if (s[2] - 2 * v) % 16 == 0 and (s[3] - 2 * v) % 16 == 0])
def test_loss_value_is_the_metric_bit_for_bit(shape, shave):
    from pesr_amd import lpips as LP
    a, b = C.image_pair(shape)
    ta, tb = _dev(a).contiguous(), _dev(b).contiguous()
    model = C.model()
    metric = LP.lpips(ta, tb, model, shave)
    loss = LP.lpips_loss(ta.clone().requires_grad_(), tb, model, shave)
    assert loss.dtype == torch.float64 and loss.shape == (shape[0],) and loss.requires_grad
    assert torch.equal(loss.detach(), metric), (loss.tolist(), metric.tolist())
    assert torch.equal(LP.lpips_loss(ta, tb, model, shave), metric)                               # without a graph too
    want = C.metric_f64(shape, shave)
    assert float(np.max(np.abs(metric.cpu().numpy() - want) / want)) <= C.SCORE_RTOL             # and lpips() is what it was
    cl = ta.contiguous(memory_format=torch.channels_last)
    assert torch.equal(LP.lpips_loss(cl, tb, model, shave), metric)                               # whatever the layout


def test_metric_cases_include_shapes_the_loss_accepts():
    ok = [(s, v) for (s, v) in C.METRIC_CASES if (s[2] - 2 * v) % 16 == 0 and (s[3] - 2 * v) % 16 == 0]
    assert ((1, 3, 16, 16), 0) in ok and ((1, 3, 64, 48), 0) in ok


def test_loss_refusals_on_the_device():
    from pesr_amd import lpips as LP
    model = C.model()
    x = torch.zeros(1, 3, 24, 20, device=DEV)
    with pytest.raises(ValueError, match=r"24 x 20 .*multiples of 16 .*max-pool backward takes even sides only"):
        LP.lpips_loss(x, x, model)
    y = torch.zeros(1, 3, 40, 40, device=DEV)
    with pytest.raises(ValueError, match="multiples of 16"):
        LP.lpips_loss(y, y, model, shave=3)
    assert LP.lpips_loss(y, y, model, shave=4).shape == (1,)         # 32 x 32


# ---- the whole gradient ------------------------------------------------------------------------------------------------------------
def _device_grad(sr, hr, model, mode_at_backward=None):
    from pesr_amd import lpips as LP
    from pesr_amd import ops
    x = _dev(sr).contiguous().requires_grad_()
    total = LP.lpips_loss(x, _dev(hr), model).sum()
    old = (ops.PRECISION, ops.BF16_MIN_WGS, ops.BF16X3_MIN_WGS)
    if mode_at_backward is not None:
        ops.set_precision(mode_at_backward)
        ops.BF16_MIN_WGS = ops.BF16X3_MIN_WGS = 1                     # as tests/test_bf16_gpu.py: these small shapes WOULD take those kernels
    try:
        n, _, h, w = sr.shape
        if mode_at_backward == "bf16":                               # conv1_2's input gradient, if it followed the mode
            assert ops.conv3x3_family_dgrad(n, h, w, 64, 64, 1, False).name == "bf16"
        if mode_at_backward == "split-bf16":                         # conv2_2's
            assert ops.conv3x3_family_dgrad(n, h // 2, w // 2, 128, 128, 1, False).name == "split-bf16"
        total.backward()
        assert ops.PRECISION == (mode_at_backward or old[0])         # the nodes restore what they found
    finally:
        ops.PRECISION, ops.BF16_MIN_WGS, ops.BF16X3_MIN_WGS = old
    return x.grad, float(total)


@pytest.mark.parametrize("shape,seed", T.TRUNK_CASES)
def test_trunk_gradient_against_float64(shape, seed):
    """d(sum of scores) / d(sr): the device against the float64 CPU trunk.  The allowance is helpers.grads_vs_fp64's rule for one
    tensor: 3 x the error of the CPU's float32 trunk against the same float64 run (never below 1e-6), each relative to the gradient's
    maximum.  Seeds: tests/lpips_trunk_grad.py TRUNK_CASES - (1,3,16,16): 6, (2,3,16,16): 11, (1,3,32,48): 0, (2,3,32,48): 4 - chosen on
    the CPU: no pool window of the float64 run has a tie and no pre-activation within 1e-4 of zero carries more than 1 % of a layer's
    gradient mass (both asserted here on the reference itself)."""
    r = T.reference(shape, seed)
    assert r["ties"] == 0 and r["kink_mass"] <= T.KINK_MASS and T.holds(r), r
    model = C.model()
    got, total = _device_grad(r["sr"], r["hr"], model)
    assert got.shape == tuple(shape) and got.dtype == torch.float32
    e_ours = float(np.abs(got.double().cpu().numpy() - r["g64"]).max() / r["gmax"])
    tol = max(3.0 * r["e_ref"], 1e-6)
    print(f"{shape} seed {seed}: device error {e_ours:.3e} of the gradient's maximum {r['gmax']:.3e}, CPU float32 trunk {r['e_ref']:.3e}, "
          f"allowance {tol:.3e}; sum of scores {total!r}")
    assert np.isfinite(e_ours) and e_ours <= tol
    again, _ = _device_grad(r["sr"], r["hr"], model)
    assert torch.equal(again, got)                                    # the same bits on every call


def test_trunk_gradient_does_not_depend_on_the_mode_at_backward():
    """--precision bf16 / split-bf16: the trunk's backward runs later, inside the step's backward, under whatever mode is set then; its
    conv nodes carry the fp32 mode, so the bits are those of an fp32 run - and another network's node still follows the mode."""
    from pesr_amd import functional as PF
    from pesr_amd import ops
    shape, seed = T.TRUNK_CASES[-1]
    r = T.reference(shape, seed)
    model = C.model()
    base, _ = _device_grad(r["sr"], r["hr"], model)
    for mode in ("bf16", "split-bf16"):
        got, _ = _device_grad(r["sr"], r["hr"], model, mode_at_backward=mode)
        assert torch.equal(got, base), mode
    # a node WITHOUT the argument dispatches by the mode, as before: the same conv under bf16 gives other bits
    conv = model.convs[1]
    x = torch.rand(2, 32, 48, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    outs = {}
    old = (ops.PRECISION, ops.BF16_MIN_WGS)
    try:
        ops.BF16_MIN_WGS = 1
        for mode in ("fp32", "bf16"):
            ops.set_precision(mode)
            xi = x.clone().requires_grad_()
            PF.conv3x3(xi, conv.weight, conv.bias, conv.packed, act=ops.ACT_RELU).sum().backward()
            outs[mode] = xi.grad
            xi = x.clone().requires_grad_()
            PF.conv3x3(xi, conv.weight, conv.bias, conv.packed, act=ops.ACT_RELU, precision="fp32").sum().backward()
            outs[mode + "/fp32"] = xi.grad
    finally:
        ops.PRECISION, ops.BF16_MIN_WGS = old
    assert not torch.equal(outs["bf16"], outs["fp32"])
    assert torch.equal(outs["bf16/fp32"], outs["fp32"]) and torch.equal(outs["fp32/fp32"], outs["fp32"])


# ---- the training step -------------------------------------------------------------------------------------------------------------
# (off, on beside the other logs, and captured: tests/test_loss_terms_gpu.py, for every term, on this harness)
BATCH = 4                                                           # as tests/test_resume_gpu.py; the HR side is 32
H = HS.harness(150, BATCH)                                          # 64 channels, 2 blocks, LR 8 x 8, lr 5e-5


def test_step_with_the_term_on():
    from pesr_amd import lpips as LP
    model = HS.lpips_model()                                         # LpipsModel.random(C.MODEL_SEED), as C.model()
    lr, hr = H.data()[0]
    tr = H.trainer(lpips_model=model, alpha_lpips=1.0)
    with torch.no_grad():
        sr0 = tr.G(lr)                                               # the sr of the first step: G before its update
        want = LP.lpips(sr0, hr, model).mean().float().item()
    logs = HS.logs(tr.gan_step(lr, hr))
    assert logs["lpips"] == want and want > 0, (logs["lpips"], want)
    logs0, states0, _ = H.run(2)
    logs4, states4, _ = H.run(4, lpips_model=model, alpha_lpips=1.0)
    assert logs4[0]["lpips"] == want
    st = HS.state(tr)
    HS.assert_only_G_moved(logs4[0], st, logs0[0], states0[0])
    assert torch.equal(st["G"], states4[0]["G"])
    # half the weight: the logged term is half (the same sr), and G moves to yet another place
    tr_half = H.trainer(lpips_model=model, alpha_lpips=0.5)
    assert HS.logs(tr_half.gan_step(lr, hr))["lpips"] == 0.5 * want
    assert not torch.equal(HS.state(tr_half)["G"], st["G"])
