"""GPU: the channel LayerNorm in front of the window attention (--wattn_norm ln, docs/modes.md section 4x) - the two kernels against the
float64 restatement of tests/layernorm_oracle.py (every group width, several pieces per lane, more pixels than one step of the grid,
large means, zero rows, locality, determinism), the autograd node, the WindowAttention module with its norm and a Generator EXACTLY
AS INITIALISED against float64 torch restatements, train steps (eager, captured, resumed, with the moving average) and test.py's loader.

Margins measured on the MI355X (observed / allowed per output; the allowed figure is 4 x the fp32 reference error of the case with a
floor of 8 * 2^-24 = 4.8e-7): see docs/experiments/layernorm.md."""
import numpy as np
import pytest
import torch

import layernorm_oracle as O
import test_window_attention_gpu as W          # (its helpers: the module rule, the train-step data and state comparisons)
from helpers import dis_sd, gen_sd
from oracle import detrand

pytestmark = pytest.mark.gpu

_SHARED = {}
CASES = [(1, 16),            # the smallest group the Generator can meet: four lanes, one pixel
         (33, 20),           # C no multiple of 16: a group of eight lanes with three idle
         (7, 48),            # a group of sixteen lanes that is not full
         (306, 64),
         (65, 256),          # one pixel per wave, P odd against the workgroup's four
         (65, 384),          # two pieces per lane, the second half idle in half the lanes
         (5, 1024)]          # four pieces per lane: the cap


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _run(c):
    """-> (y, dx, dgamma, dbeta) of the two ops"""
    from pesr_amd import ops
    x, gamma, beta, dy = (_cuda(c[k]) for k in ("x", "gamma", "beta", "dy"))
    y, stats = ops.layernorm_fwd(x, gamma, beta)
    assert stats.shape == (x.shape[0], 2) and stats.dtype == torch.float32
    return (y,) + tuple(ops.layernorm_bwd(x, gamma, stats, dy))


def _check(case, c, what):
    got = dict(zip(O.NAMES, _run(c)))
    bad = []
    for name in O.NAMES:
        assert bool(torch.isfinite(got[name]).all()), (what, case, name)
        err, tol = O.rel_err(got[name], c["want"][name]), O.tolerance(c["ref"][name])
        print(f"{what} {case} {name}: observed {err:.2e} / allowed {tol:.2e} (fp32 reference error {c['ref'][name]:.2e})")
        if not err <= tol:
            bad.append((name, err, tol))
    assert not bad, (what, case, bad)


# ---- 1. the kernels against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernels_against_float64(case):
    """Per output (y, dx, dgamma, dbeta), the maximum error over the float64 maximum within 4 x the fp32 reference error of the same
    case (the oracle run in float32 on the CPU), with a floor of 8 * 2^-24."""
    _check(case, O.case(*case), "kernel")


def test_more_pixels_than_one_step_of_the_grid():
    """C = 16 with P beyond what the capped grid covers in one step (asked of the library): every workgroup walks on, the last step is
    ragged, and each lane's channel sums run over several pixels."""
    from pesr_amd import ops
    one_pass = ops.layernorm_pass_pixels(1 << 22, 16)
    P = one_pass + 4133
    assert ops.layernorm_partials(P, 16) == ops.layernorm_partials(1 << 22, 16) and ops.layernorm_pass_pixels(P, 16) == one_pass < P
    assert P * 16 * 4 < 32 << 20
    _check((P, 16), O.case(P, 16), "strided")


# ---- 2. inputs that break naive forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(65, 256, "big-mean"), (7, 48, "big-mean"), (65, 256, "features")], ids=lambda c: "-".join(map(str, c)))
def test_large_means(case):
    """x = 1000 + n, and x = 13 + 40 n (the trunk's features in front of a block): a one-pass E[x^2] - mean^2 in fp32 is off by a tenth
    of the output's maximum on the first (tests/test_layernorm_cpu.py shows it); the centred form stays within the kernels' rule."""
    _check(case, O.case(*case), "large mean")


@pytest.mark.parametrize("case", [(7, 16), (65, 256), (10, 384)], ids=str)
def test_zero_rows_give_beta_exactly_and_everything_stays_finite(case):
    c = O.case(*case, "zero-rows")
    y, dx, dgamma, dbeta = _run(c)
    rows = y[::3]
    assert torch.equal(rows, _cuda(c["beta"]).expand_as(rows))
    _check(case, c, "zero rows")


# ---- 3. locality -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(33, 20, 17), (65, 256, 64), (10, 384, 3)], ids=str)
def test_a_pixel_sees_nothing_but_itself(case):
    P, C, pix = case
    a = O.case(P, C)
    x2 = a["x"].copy()
    x2[pix] = O.normal_like((C,), 4242) * np.float32(3.0) + np.float32(2.0)
    b = dict(a, x=x2)
    (ya, dxa, _, _), (yb, dxb, _, _) = _run(a), _run(b)
    others = torch.ones(P, dtype=torch.bool, device="cuda")
    others[pix] = False
    assert torch.equal(ya[others], yb[others]) and not torch.equal(ya[pix], yb[pix])
    assert torch.equal(dxa[others], dxb[others]) and not torch.equal(dxa[pix], dxb[pix])


# ---- 4. determinism and the precision modes ------------------------------------------------------------------------------------------------
def test_same_bits_on_every_run_and_in_every_precision_mode():
    from pesr_amd import ops
    c = O.case(306, 64)
    first = _run(c)
    assert all(t.dtype == torch.float32 for t in first)
    for mode in ops.PRECISIONS:
        with ops.use_precision(mode):
            again = _run(c)
        for name, f, g in zip(O.NAMES, first, again):
            assert torch.equal(f, g), (mode, name)
    # every output is written once per element with no zero-fill in front: poisoned buffers change nothing (torch's allocator hands the
    # next empty tensor of a size the block just freed)
    del again, f, g
    poison = [torch.full_like(t, float("nan")) for t in first]
    del poison
    for name, f, g in zip(O.NAMES, first, _run(c)):
        assert torch.equal(f, g), name


# ---- 5. the autograd node ------------------------------------------------------------------------------------------------------------------
def test_autograd_node_and_refusals():
    from pesr_amd import functional as PF
    from pesr_amd import ops
    c = O.case(306, 64)
    x = _cuda(c["x"]).reshape(2, 9, 17, 64).requires_grad_(True)
    gamma, beta = _cuda(c["gamma"]).requires_grad_(True), _cuda(c["beta"]).requires_grad_(True)
    y = PF.LayerNormFn.apply(x, gamma, beta)
    y.backward(_cuda(c["dy"]).reshape(2, 9, 17, 64))
    want = _run(c)
    assert y.shape == x.shape and torch.equal(y.reshape(306, 64), want[0])
    assert torch.equal(x.grad.reshape(306, 64), want[1]) and torch.equal(gamma.grad, want[2]) and torch.equal(beta.grad, want[3])
    xd, g, b = x.detach(), gamma.detach(), beta.detach()
    _, stats = ops.layernorm_fwd(xd, g, b)
    with pytest.raises(ValueError, match="C = 18"):
        ops.layernorm_fwd(torch.zeros(4, 18, device="cuda"), torch.ones(18, device="cuda"), torch.zeros(18, device="cuda"))
    with pytest.raises(ValueError, match="C = 1028"):
        ops.layernorm_fwd(torch.zeros(4, 1028, device="cuda"), torch.ones(1028, device="cuda"), torch.zeros(1028, device="cuda"))
    with pytest.raises(ValueError, match="gamma"):
        ops.layernorm_fwd(xd, torch.ones(32, device="cuda"), b)
    with pytest.raises(ValueError, match="beta"):
        ops.layernorm_fwd(xd, g, torch.zeros(64, 1, device="cuda"))
    with pytest.raises(ValueError, match="stats"):
        ops.layernorm_bwd(xd, g, stats[:-1], xd)
    with pytest.raises(ValueError, match="dy"):
        ops.layernorm_bwd(xd, g, stats, xd[:1])
    with pytest.raises(Exception, match="float32"):
        ops.layernorm_fwd(xd.double(), g, b)


# ---- 6. the module against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_module_against_float64(shift):
    """The existing module test's setup and bounds (tests/test_window_attention_gpu.py), with the norm in front of qkv and a weight and
    bias of the norm that are not the initial 1 and 0."""
    from pesr_amd.model.basic import WindowAttention
    torch.manual_seed(21)
    blk = WindowAttention(64, 64, shift=shift, norm="ln")
    with torch.no_grad():
        blk.qkv.weight[:128] *= 4.0
        blk.norm.weight.copy_(torch.as_tensor(1.0 + 0.5 * O.normal_like((64,), 31)))
        blk.norm.bias.copy_(torch.as_tensor(0.3 * O.normal_like((64,), 32)))
    blk.cuda()
    x = np.ascontiguousarray(O.WO.CO.features((2, 12, 20, 64), 51, scale=1.0, offset=0.3).transpose(0, 3, 1, 2))
    W._module_vs_float64(blk, x, lambda sd, x64: O.block(sd, x64, shift), f"WindowAttention(shift={shift}, norm=ln)")
    assert [k for k, _ in blk.named_parameters()] == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "norm.weight", "norm.bias"]


# ---- 7. the Generator exactly as initialised against float64 ---------------------------------------------------------------------------------
def _generator_errors(opt, seed=6):
    """tests/test_window_attention_gpu.py's _generator_errors with the norm and WITHOUT any scaling of q and k: a Generator on a
    [1, 3, 12, 20] image of grey levels against its float64 restatement -> (the Generator, {name: (observed, fp32 reference error)},
    the first block's largest logit in float64, the largest feature in front of the blocks)."""
    from pesr_amd.model import Generator
    torch.manual_seed(seed)
    G = Generator(opt)
    G.load_state_dict(gen_sd(opt["num_channels"], opt["depth"], 0), strict=False)   # seeded conv weights; the attention keeps its seeded initialisation
    x = detrand.image_batch((1, 3, 12, 20), 61)
    ref, taps = {}, {}
    for dtype in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in G.state_dict().items()}
        y = O.generator(sd, x.to(dtype), opt["depth"], 0.1, taps if dtype == torch.float64 else None)
        if dtype == torch.float64:
            target = torch.as_tensor(O.WO.CO.features(tuple(y.shape), 55, scale=float(y.detach().abs().mean()), offset=0.0))
        (y - target.to(dtype)).abs().mean().backward()
        ref[dtype] = (y.detach().double(), {k: v.grad.double() for k, v in sd.items()})
    y64, g64 = ref[torch.float64]
    y32, g32 = ref[torch.float32]
    top = O.largest_logit(taps["qkv.0"], 0)
    feat = max(float(taps[k].abs().max()) for k in taps if k.startswith("in."))
    G.cuda()
    y = G(x.cuda())
    (y - target.cuda()).abs().mean().backward()
    out = {"output": (float((y.detach().cpu().double() - y64).abs().max()), float((y32 - y64).abs().max()))}
    for k, p in G.named_parameters():
        assert p.grad is not None and float(g64[k].abs().max()) > 0, k
        out[k] = (O.rel_err(p.grad, g64[k]), O.rel_err(g32[k], g64[k]))
    return G, out, top, feat


@pytest.mark.parametrize("ca", [False, True], ids=["alone", "with-ca"])
def test_generator_as_initialised_against_float64(ca):
    """What the norm exists for.  The existing Generator test scales q and k by 1/16, because without it the logits reach 2600 and no two
    fp32 evaluations agree to rounding; with the norm in front of qkv the logits of the Generator exactly as constructed stay of the
    order of 1 (asserted: below 40) and the comparison holds with that test's bounds: the output within max(2e-3 grey levels, 4 x the
    fp32 reference error), every parameter gradient - norm.* included - within max(1e-4, 4 x its reference error) of its maximum."""
    from pesr_amd.model.basic import ChannelLayerNorm
    opt = {"num_channels": 64, "depth": 2, "res_scale": 0.1, "wattn_every": 1, "wattn_dim": 64, "wattn_norm": "ln"}
    if ca:
        opt.update(attention="ca", ca_reduction=4)
    G, errs, top, feat = _generator_errors(opt)
    assert [m.shift for m in G.wattn.values()] == [0, 4] and all(isinstance(m.norm, ChannelLayerNorm) for m in G.wattn.values())
    what = f"Generator({'ca' if ca else 'plain'}, ln)"
    print(f"{what}: largest logit of the first block {top:.2f}, largest feature in front of a block {feat:.0f}")
    assert top < 40.0, top
    assert {"wattn.0.norm.weight", "wattn.0.norm.bias", "wattn.1.norm.weight", "wattn.1.norm.bias"} <= set(errs)
    bad = []
    for k, (got, ref) in errs.items():
        allowed = max(4.0 * ref, 2e-3 if k == "output" else 1e-4)
        print(f"{what} {k}: observed {got:.2e} / allowed {allowed:.2e} (fp32 reference error {ref:.2e})")
        if not got <= allowed:
            bad.append((k, got, allowed))
    assert not bad, bad


# ---- 8. train steps ----------------------------------------------------------------------------------------------------------------------
G_OPT = dict(W.G_OPT, wattn_norm="ln")
NORM_KEYS = [f"wattn.{i}.norm.{p}" for i in range(W.DEPTH) for p in ("weight", "bias")]


def _generator(seed=0):
    from model import Generator
    state = torch.random.get_rng_state()
    torch.manual_seed(700 + seed)
    G = Generator(G_OPT)
    torch.random.set_rng_state(state)
    G.load_state_dict(gen_sd(W.CH, W.DEPTH, seed), strict=False)
    return G.cuda()


def _trainer(phase, seed=0, ema_decay=0.0):
    from model import Discriminator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = _generator(seed)
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=W.LR, betas=(0.9, 0.999), ema_decay=ema_decay)
    if phase == "pretrain":
        return Trainer(G, optim_G=oG)
    D = Discriminator({"patch_size": W.PS, "spectral_norm": False}); D.load_state_dict(dis_sd(W.PS, seed + 1)); D.cuda()
    return Trainer(G, D, W._vgg(), oG, FlatAdam(D.parameters(), lr=W.LR, betas=(0.9, 0.999)))


def _four_eager(phase):
    key = ("eager", phase)
    if key not in _SHARED:
        tr = _trainer(phase)
        start = {k: v.detach().clone() for k, v in tr.G.state_dict().items()}
        logs, states = [], []
        for lr, hr in W._data():
            logs.append(W._logs(W._step(tr, phase)(lr, hr)))
            states.append(W._state(tr))
        _SHARED[key] = (logs, states, start, {k: v.detach().clone() for k, v in tr.G.state_dict().items()})
    return _SHARED[key]


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_eager_steps_are_finite_and_move_the_norms(phase):
    logs, states, start, end = _four_eager(phase)
    assert all(np.isfinite(v) for l in logs for v in l.values()), logs
    assert [k for k in start if ".norm." in k] == NORM_KEYS
    for k in [k for k in start if k.startswith("wattn.")]:
        assert not torch.equal(start[k], end[k]), k
        assert bool(torch.isfinite(end[k]).all()), k


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_two_eager_steps_a_capture_and_two_replays_are_four_eager_steps(phase):
    logs4, states4, _, _ = _four_eager(phase)
    tr = _trainer(phase)
    data = W._data()
    for i in range(2):
        assert W._logs(W._step(tr, phase)(*data[i])) == logs4[i]
    step = (tr.capture_gan_step if phase == "train" else tr.capture_pretrain_step)(*data[0])
    for i in (2, 3):
        assert W._logs(step(*data[i])) == logs4[i], i
        W._assert_state(tr, states4[i], f"replay {i}")


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_resume_after_two_steps_equals_four_uninterrupted(phase, tmp_path):
    from pesr_amd import checkpoint
    logs4, states4, _, _ = _four_eager(phase)
    tr = _trainer(phase)
    data = W._data()
    for lr, hr in data[:2]:
        W._step(tr, phase)(lr, hr)
    path = str(tmp_path / "state.pt")
    saved = {"G": tr.G.state_dict(), "optim_G": tr.optim_G.state_dict()}
    if phase == "train":
        saved.update({"D": tr.D.state_dict(), "optim_D": tr.optim_D.state_dict()})
    checkpoint.atomic_save(saved, path)
    st = checkpoint.load_state(path)
    assert [k for k in st["G"] if ".norm." in k] == NORM_KEYS
    fresh = _trainer(phase, seed=40)              # other weights, zero moments
    assert not torch.equal(fresh.optim_G.flat.flat_p, states4[1]["G"])
    fresh.G.load_state_dict(st["G"]); fresh.optim_G.load_state_dict(st["optim_G"])
    if phase == "train":
        fresh.D.load_state_dict(st["D"]); fresh.optim_D.load_state_dict(st["optim_D"])
    for i in (2, 3):
        assert W._logs(W._step(fresh, phase)(*data[i])) == logs4[i], i
        W._assert_state(fresh, states4[i], f"resumed, step {i + 1}")


def test_moving_average_generator_has_norms_of_its_own():
    from pesr_amd.model.basic import ChannelLayerNorm
    tr = _trainer("pretrain", ema_decay=0.9)
    G_ema = tr.optim_G.ema_module(tr.G)
    assert sum(isinstance(m, ChannelLayerNorm) for m in G_ema.modules()) == W.DEPTH
    for lr, hr in W._data()[:2]:
        tr.pretrain_step(lr, hr)
    tr.optim_G.refresh_ema()
    live, ema = dict(tr.G.named_parameters()), dict(G_ema.named_parameters())
    for k in NORM_KEYS:
        assert live[k].data_ptr() != ema[k].data_ptr() and not torch.equal(live[k], ema[k]), k
        first = torch.ones(W.CH) if k.endswith("weight") else torch.zeros(W.CH)
        assert not torch.equal(ema[k].cpu(), first), k                               # the average moves too
    with torch.no_grad():
        out = G_ema(W._data()[0][0])
    assert out.shape == (W.BATCH, 3, 4 * W.PS, 4 * W.PS) and bool(torch.isfinite(out).all())


# ---- 9. inference plumbing -----------------------------------------------------------------------------------------------------------------
def test_loader_of_test_py_builds_the_norms_and_runs_an_odd_image_and_tiles(tmp_path):
    from pesr_amd import tile
    from pesr_amd.model import Generator
    from pesr_amd.model.basic import ChannelLayerNorm
    T = W._entry("test")
    opt = {"num_channels": 64, "depth": 2, "res_scale": 0.1}
    torch.manual_seed(8)
    G = Generator(dict(opt, wattn_every=1, wattn_dim=64, wattn_norm="ln"))
    G.load_state_dict(gen_sd(64, 2, 3), strict=False)
    with torch.no_grad():
        for i, m in enumerate(G.wattn.values()):
            m.norm.weight.copy_(torch.as_tensor(1.0 + 0.5 * O.normal_like((64,), 41 + i)))
            m.norm.bias.copy_(torch.as_tensor(0.3 * O.normal_like((64,), 51 + i)))
    path = str(tmp_path / "ln.pt")
    torch.save(G.state_dict(), path)
    loaded = T.load_generator(opt, path, 4).cuda()
    assert [(k, m.dim, m.shift, isinstance(m.norm, ChannelLayerNorm)) for k, m in loaded.wattn.items()] == [("0", 64, 0, True), ("1", 64, 4, True)]
    assert all(torch.equal(loaded.state_dict()[k].cpu(), v) for k, v in G.state_dict().items())
    G.cuda()
    img = detrand.image_batch((1, 3, 13, 9), 81).cuda()           # odd sides
    with torch.no_grad():
        out, direct = loaded(img), G(img)
        assert out.shape == (1, 3, 52, 36) and bool(torch.isfinite(out).all()) and torch.equal(out, direct)
        tiled, _ = tile.tiled_forward(loaded, img, 4, 8, 2, 4)
        assert tiled.shape == out.shape and bool(torch.isfinite(tiled).all())
