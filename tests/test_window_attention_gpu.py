"""GPU: the window self-attention blocks of the Generator (--wattn_every, docs/modes.md section 4w) - the two kernels against the
float64 restatement of tests/window_attention_oracle.py (ragged windows, several heads, saturated logits, exactness, locality,
determinism), the WindowAttention module and a Generator with such blocks against float64 torch restatements, train steps (eager,
captured, resumed, with the moving average) and test.py's loader.

Margins measured on the MI355X (observed / allowed, out and dqkv; the allowed figure is 4 x the fp32 reference error of the case with
a floor of 8 * 2^-24 = 4.8e-7): see docs/experiments/window_attention.md."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import window_attention_oracle as O
from helpers import dis_sd, gen_sd, vgg_sd
from oracle import detrand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHARED = {}
CASES = [(1, 8, 8, 32, 0),          # one full window
         (1, 8, 8, 32, 4),          # four quarter windows
         (2, 9, 17, 64, 0), (2, 9, 17, 64, 4),      # ragged edges, two heads, a second image
         (1, 13, 5, 160, 4),        # five heads: more than a workgroup's waves
         (2, 16, 24, 128, 4),
         (1, 3, 40, 32, 0)]


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_wag_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run(c, shift):
    from pesr_amd import ops
    qkv, dout = _cuda(c["qkv"]), _cuda(c["dout"])
    return ops.window_attention_fwd(qkv, shift), ops.window_attention_bwd(qkv, dout, shift)


def _check(case, c, what):
    out, dqkv = _run(c, case[4])
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    for name, got, want, ref in (("out", out, c["out"], c["ref_out"]), ("dqkv", dqkv, c["dqkv"], c["ref_dqkv"])):
        err, tol = O.rel_err(got, want), O.tolerance(ref)
        print(f"{what} {case} {name}: observed {err:.2e} / allowed {tol:.2e} (fp32 reference error {ref:.2e})")
        assert err <= tol, (what, case, name, err, tol)


# ---- 1. the kernels against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernels_against_float64(case):
    """Per tensor, the maximum error over the float64 maximum within 4 x the fp32 reference error of the same case (the oracle run in
    float32 on the CPU), with a floor of 8 * 2^-24: x 2 for two independent fp32 orderings, x 2 for a device expf that need not be
    the host's."""
    _check(case, O.case(*case), "kernel")


def test_saturated_logits():
    """q and k times 6: logits beyond 100, where a softmax without the row maximum overflows.  The reference error is larger because the
    logits are (their fp32 rounding error goes through exp), which is why the bound is relative to it."""
    case = (1, 8, 8, 32, 0)
    c = O.case(*case, qk_scale=6.0)
    parts = []
    O.attention(torch.as_tensor(c["qkv"]).double(), 0, parts)
    top = max(float(S.max()) for _, _, S in parts)
    assert top > 100.0 and not np.isfinite(np.exp(np.float32(top))), top
    _check(case, c, f"saturated (largest logit {top:.0f})")


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 1, 1, 32, 0), (1, 1, 1, 64, 4)], ids=str)
def test_a_single_pixel_attends_to_itself_exactly(case):
    N, H, W, D, s = case
    c = dict(qkv=O.normal_like((N, H, W, 3 * D), 77 + D), dout=O.normal_like((N, H, W, D), 78 + D))
    out, dqkv = _run(c, s)
    assert torch.equal(out.cpu(), torch.as_tensor(c["qkv"][..., 2 * D:]))            # out == v
    assert torch.equal(dqkv[..., 2 * D:].cpu(), torch.as_tensor(c["dout"]))          # dv == dout
    assert bool((dqkv[..., :2 * D] == 0).all())                                     # dq, dk


# ---- 3. locality -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
def test_a_window_sees_nothing_outside_itself(shift):
    N, H, W, D = 1, 16, 16, 64
    # a whole window, so both lane halves hold tokens: the last one at shift 0 (rows and columns 8 .. 15); at shift 4 the middle one
    # of the 3 x 3 grid (4 .. 11), which has neighbours on all sides
    rows, cols = O.windows(H, W, shift)[-1 if shift == 0 else 4]
    assert (rows[0], rows[-1], cols[0], cols[-1]) == ((8, 15, 8, 15) if shift == 0 else (4, 11, 4, 11))
    inside = np.zeros((N, H, W, 1), dtype=bool)
    inside[:, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = True
    a = dict(qkv=O.normal_like((N, H, W, 3 * D), 91), dout=O.normal_like((N, H, W, D), 92))
    b = dict(qkv=np.where(inside, a["qkv"], O.normal_like((N, H, W, 3 * D), 93)), dout=a["dout"])
    c = dict(qkv=a["qkv"], dout=np.where(inside, a["dout"], O.normal_like((N, H, W, D), 94)))
    (oa, ga), (ob, _), (_, gc) = _run(a, shift), _run(b, shift), _run(c, shift)
    m = torch.as_tensor(inside).cuda()
    assert torch.equal(oa[m.expand_as(oa)], ob[m.expand_as(ob)]) and not torch.equal(oa, ob)
    assert torch.equal(ga[m.expand_as(ga)], gc[m.expand_as(gc)]) and not torch.equal(ga, gc)


# ---- 4. determinism and the precision modes ------------------------------------------------------------------------------------------------
def test_same_bits_on_every_run_and_in_every_precision_mode():
    from pesr_amd import ops
    case = (2, 16, 24, 128, 4)
    c = O.case(*case)
    first = _run(c, 4)
    assert first[0].dtype == torch.float32 and first[1].dtype == torch.float32
    for mode in ops.PRECISIONS:
        with ops.use_precision(mode):
            again = _run(c, 4)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), mode
    # dqkv is written once per element with no zero-fill in front: a poisoned output buffer changes nothing (torch's allocator hands
    # the next empty tensor of this size the block just freed)
    del again
    torch.full_like(first[1], float("nan"))
    assert torch.equal(_run(c, 4)[1], first[1])


def test_autograd_node_and_refusals():
    from pesr_amd import functional as PF
    from pesr_amd import ops
    c = O.case(2, 9, 17, 64, 4)
    qkv = _cuda(c["qkv"]).requires_grad_(True)
    out = PF.WindowAttentionFn.apply(qkv, 4)
    out.backward(_cuda(c["dout"]))
    want = _run(c, 4)
    assert torch.equal(out, want[0]) and torch.equal(qkv.grad, want[1])
    with pytest.raises(ValueError, match="shift"):
        ops.window_attention_fwd(qkv.detach(), 8)
    with pytest.raises(ValueError, match="3 D"):
        ops.window_attention_fwd(torch.zeros(1, 8, 8, 48, device="cuda"))
    with pytest.raises(ValueError, match="dout"):
        ops.window_attention_bwd(qkv.detach(), torch.zeros(2, 9, 17, 32, device="cuda"), 4)


# ---- 5. the module and the Generator against float64 -----------------------------------------------------------------------------------------
def _module_vs_float64(module, x, forward64, what):
    """The rule of tests/test_channel_attention_gpu.py's _module_vs_float64: the output within atol + 1e-5 |ref|, every parameter gradient
    of an L1 loss against a fixed seeded target within 1e-4 of its tensor's maximum.  atol: that file allows 2e-3 on ResBlock outputs of
    magnitude 40, that is 5e-5 of the output's scale - here the same fraction of this output's float64 maximum.  -> the input gradient."""
    xg = _cuda(x).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = module(xg)
    sd = O.CO.double_leaves(module.state_dict())
    x64 = torch.as_tensor(x).double().requires_grad_(True)
    y64 = forward64(sd, x64)
    atol = 5e-5 * float(y64.detach().abs().max())
    err = (y.detach().cpu().double() - y64.detach()).abs()
    print(f"{what} output: {float(err.max()):.2e} (atol {atol:.2e})")
    assert bool((err <= atol + 1e-5 * y64.detach().abs()).all()), (what, float(err.max()), atol)
    target = torch.as_tensor(O.CO.features(tuple(y64.shape), 55, scale=float(y64.detach().abs().mean()), offset=0.0))
    (y - target.cuda()).abs().mean().backward()
    (y64 - target.double()).abs().mean().backward()
    for k, p in module.named_parameters():
        assert p.grad is not None and sd[k].grad is not None and float(sd[k].grad.abs().max()) > 0, k
        e = O.rel_err(p.grad, sd[k].grad)
        print(f"{what} {k}: {e:.2e}")
        assert e <= 1e-4, (what, k, e)
    e = O.rel_err(xg.grad, x64.grad)
    print(f"{what} input gradient: {e:.2e}")
    assert e <= 1e-4, (what, e)


@pytest.mark.parametrize("shift", [0, 4])
def test_module_against_float64(shift):
    from pesr_amd.model.basic import WindowAttention
    torch.manual_seed(21)
    blk = WindowAttention(64, 64, shift=shift).cuda()
    with torch.no_grad():          # (sharper logits than the initialisation's: the softmax is far from uniform)
        blk.qkv.weight[:128] *= 4.0
    x = np.ascontiguousarray(O.CO.features((2, 12, 20, 64), 51, scale=1.0, offset=0.3).transpose(0, 3, 1, 2))
    _module_vs_float64(blk, x, lambda sd, x64: O.block(sd, x64, shift), f"WindowAttention(shift={shift})")
    assert [k for k, _ in blk.named_parameters()] == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"]


def _generator_errors(opt, seed=6, qk_gain=1.0):
    """A Generator on a [1, 3, 12, 20] image of grey levels against its float64 restatement -> (the Generator, {name: (observed, fp32
    reference error)}): "output" in grey levels, every parameter's gradient of an L1 loss against a fixed seeded target as the maximum
    error over the float64 maximum.  The fp32 reference error is the same restatement evaluated in float32 on the CPU."""
    from pesr_amd.model import Generator
    torch.manual_seed(seed)
    G = Generator(opt)
    G.load_state_dict(gen_sd(opt["num_channels"], opt["depth"], 0), strict=False)   # seeded conv weights; the attention keeps its seeded initialisation
    with torch.no_grad():
        for blk in G.wattn.values():          # q and k (weights and biases) times qk_gain each: see test_generator_against_float64
            blk.qkv.weight[:2 * blk.dim] *= qk_gain
            blk.qkv.bias[:2 * blk.dim] *= qk_gain
    x = detrand.image_batch((1, 3, 12, 20), 61)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in G.state_dict().items()}
        y = O.generator(sd, x.to(dtype), opt["depth"], 0.1)
        if dtype == torch.float64:
            target = torch.as_tensor(O.CO.features(tuple(y.shape), 55, scale=float(y.detach().abs().mean()), offset=0.0))
        (y - target.to(dtype)).abs().mean().backward()
        ref[dtype] = (y.detach().double(), {k: v.grad.double() for k, v in sd.items()})
    y64, g64 = ref[torch.float64]
    y32, g32 = ref[torch.float32]
    # the first block's logits, in float64
    with torch.no_grad():
        sd = {k: v.detach().double() for k, v in G.state_dict().items()}
        c = lambda k, v, p: torch.nn.functional.conv2d(v, sd[k + ".weight"], sd[k + ".bias"], padding=p)
        h = O.CO.resblock(sd, c("embed", c("sub_mean", x.double(), 0), 1), 0.1, "body.0.")
        parts = []
        O.attention(c("wattn.0.qkv", h, 1).permute(0, 2, 3, 1), 0, parts)
    top = max(float(S.abs().max()) for _, _, S in parts)
    G.cuda()
    y = G(x.cuda())
    (y - target.cuda()).abs().mean().backward()
    out = {"output": (float((y.detach().cpu().double() - y64).abs().max()), float((y32 - y64).abs().max()))}
    for k, p in G.named_parameters():
        assert p.grad is not None and float(g64[k].abs().max()) > 0, k
        out[k] = (O.rel_err(p.grad, g64[k]), O.rel_err(g32[k], g64[k]))
    return G, out, top


@pytest.mark.parametrize("ca", [False, True], ids=["alone", "with-ca"])
def test_generator_against_float64(ca):
    """The bounds of the channel attention file's Generator test - the output within 2e-3 grey levels, every parameter gradient within
    1e-4 of its tensor's maximum - or, where that is larger, the kernel tests' rule: 4 x the fp32 reference error of the same case (this
    restatement in float32 on the CPU).
    The inputs are chosen so that the comparison means something.  With the seeded initialisation as it stands the features of a
    grey-level image reach 160, q and k reach 100 and the logits 2600 (float64): the softmax is an argmax, a rounding error of 2^-24
    of a logit is 1.5e-4 in the exponent and near-ties between keys flip - any two fp32 evaluations then differ by jumps, not by
    rounding (measured: this path 5e-4 .. 3.5e-3 grey levels from float64, the float32 CPU restatement 1e-4 .. 1e-3, gradients up to
    7e-3 of their maximum; docs/experiments/window_attention.md).  So q and k are scaled by 1/16 each, which brings the logits to about
    10: asserted below to lie between 2 and 40, neither a uniform nor a saturated softmax."""
    opt = {"num_channels": 64, "depth": 2, "res_scale": 0.1, "wattn_every": 1, "wattn_dim": 64}
    if ca:
        opt.update(attention="ca", ca_reduction=4)
    G, errs, top = _generator_errors(opt, qk_gain=1.0 / 16)
    assert [m.shift for m in G.wattn.values()] == [0, 4]
    print(f"Generator({'ca' if ca else 'plain'}): largest logit of the first block {top:.1f}")
    assert 2.0 < top < 40.0, top
    bad = []
    for k, (got, ref) in errs.items():
        allowed = max(4.0 * ref, 2e-3 if k == "output" else 1e-4)
        print(f"Generator({'ca' if ca else 'plain'}) {k}: observed {got:.2e} / allowed {allowed:.2e} (fp32 reference error {ref:.2e})")
        if not got <= allowed:
            bad.append((k, got, allowed))
    assert not bad, bad


# ---- 6. train steps ----------------------------------------------------------------------------------------------------------------------
CH, DEPTH, PS, BATCH, LR = 64, 2, 8, 2, 5e-5
G_OPT = {"num_channels": CH, "depth": DEPTH, "res_scale": 0.1, "scale": 4, "wattn_every": 1, "wattn_dim": 64}


def _vgg():
    if "vgg" not in _SHARED:
        from model import VGG
        V = VGG(); V.load_state_dict(vgg_sd()); V.cuda()
        _SHARED["vgg"] = V
    return _SHARED["vgg"]


def _data():
    if "data" not in _SHARED:
        _SHARED["data"] = [(detrand.image_batch((BATCH, 3, PS, PS), 250 + i).cuda(),
                            detrand.image_batch((BATCH, 3, 4 * PS, 4 * PS), 260 + i).cuda()) for i in range(4)]
    return _SHARED["data"]


def _generator(seed=0):
    from model import Generator
    state = torch.random.get_rng_state()
    torch.manual_seed(700 + seed)
    G = Generator(G_OPT)
    torch.random.set_rng_state(state)
    G.load_state_dict(gen_sd(CH, DEPTH, seed), strict=False)
    return G.cuda()


def _trainer(phase, seed=0, ema_decay=0.0):
    from model import Discriminator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = _generator(seed)
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=LR, betas=(0.9, 0.999), ema_decay=ema_decay)
    if phase == "pretrain":
        return Trainer(G, optim_G=oG)
    D = Discriminator({"patch_size": PS, "spectral_norm": False}); D.load_state_dict(dis_sd(PS, seed + 1)); D.cuda()
    return Trainer(G, D, _vgg(), oG, FlatAdam(D.parameters(), lr=LR, betas=(0.9, 0.999)))


def _state(tr):
    st = {"G": tr.optim_G.flat.flat_p.clone(), "G.exp_avg": tr.optim_G.exp_avg.clone(), "G.exp_avg_sq": tr.optim_G.exp_avg_sq.clone()}
    if tr.D is not None:
        st.update({"D": tr.optim_D.flat.flat_p.clone(), **{"D." + k: v.clone() for k, v in tr.D.state_dict().items()}})
    return st


def _logs(d):
    return {k: v.item() for k, v in d.items()}


def _step(tr, phase):
    return tr.gan_step if phase == "train" else tr.pretrain_step


def _four_eager(phase):
    key = ("eager", phase)
    if key not in _SHARED:
        tr = _trainer(phase)
        start = {k: v.detach().clone() for k, v in tr.G.state_dict().items()}
        logs, states = [], []
        for lr, hr in _data():
            logs.append(_logs(_step(tr, phase)(lr, hr)))
            states.append(_state(tr))
        _SHARED[key] = (logs, states, start, {k: v.detach().clone() for k, v in tr.G.state_dict().items()})
    return _SHARED[key]


def _assert_state(tr, want, what):
    got = _state(tr)
    assert sorted(got) == sorted(want)
    for k in got:
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_eager_steps_are_finite_and_move_the_blocks(phase):
    logs, states, start, end = _four_eager(phase)
    assert all(np.isfinite(v) for l in logs for v in l.values()), logs
    wa = [k for k in start if k.startswith("wattn.")]
    assert len(wa) == 4 * DEPTH
    for k in wa:
        assert not torch.equal(start[k], end[k]), k
        assert bool(torch.isfinite(end[k]).all()), k


def test_discriminator_step_is_the_same_bits_for_the_same_generator():
    _, states, _, _ = _four_eager("train")
    tr = _trainer("train")
    tr.gan_step(*_data()[0])
    _assert_state(tr, states[0], "second run, step 1")


@pytest.mark.parametrize("phase", ["pretrain", "train"])
def test_two_eager_steps_a_capture_and_two_replays_are_four_eager_steps(phase):
    logs4, states4, _, _ = _four_eager(phase)
    tr = _trainer(phase)
    data = _data()
    for i in range(2):
        assert _logs(_step(tr, phase)(*data[i])) == logs4[i]
    step = (tr.capture_gan_step if phase == "train" else tr.capture_pretrain_step)(*data[0])
    for i in (2, 3):
        assert _logs(step(*data[i])) == logs4[i], i
        _assert_state(tr, states4[i], f"replay {i}")


def test_moving_average_generator_has_blocks_of_its_own():
    from pesr_amd.model.basic import WindowAttention
    tr = _trainer("pretrain", ema_decay=0.9)
    G_ema = tr.optim_G.ema_module(tr.G)
    assert [(m.dim, m.shift) for m in G_ema.modules() if isinstance(m, WindowAttention)] == [(64, 0), (64, 4)]
    for lr, hr in _data()[:2]:
        tr.pretrain_step(lr, hr)
    tr.optim_G.refresh_ema()
    live, ema = dict(tr.G.named_parameters()), dict(G_ema.named_parameters())
    wa = [k for k in live if k.startswith("wattn.")]
    assert len(wa) == 4 * DEPTH
    for k in wa:
        assert not torch.equal(live[k], ema[k]), k
    with torch.no_grad():
        out = G_ema(_data()[0][0])
    assert out.shape == (BATCH, 3, 4 * PS, 4 * PS) and bool(torch.isfinite(out).all())


def test_resume_after_two_steps_equals_four_uninterrupted(tmp_path):
    from pesr_amd import checkpoint
    logs4, states4, _, _ = _four_eager("train")
    tr = _trainer("train")
    data = _data()
    for lr, hr in data[:2]:
        tr.gan_step(lr, hr)
    path = str(tmp_path / "state.pt")
    checkpoint.atomic_save({"G": tr.G.state_dict(), "D": tr.D.state_dict(), "optim_G": tr.optim_G.state_dict(),
                            "optim_D": tr.optim_D.state_dict()}, path)
    st = checkpoint.load_state(path)
    assert any(k.startswith("wattn.") for k in st["G"])
    fresh = _trainer("train", seed=40)              # other weights, zero moments
    assert not torch.equal(fresh.optim_G.flat.flat_p, states4[1]["G"])
    fresh.G.load_state_dict(st["G"]); fresh.D.load_state_dict(st["D"])
    fresh.optim_G.load_state_dict(st["optim_G"]); fresh.optim_D.load_state_dict(st["optim_D"])
    for i in (2, 3):
        assert _logs(fresh.gan_step(*data[i])) == logs4[i], i
        _assert_state(fresh, states4[i], f"resumed, step {i + 1}")


# ---- 7. inference plumbing -----------------------------------------------------------------------------------------------------------------
def test_loader_of_test_py_runs_an_odd_image_the_ensemble_and_tiles(tmp_path):
    from pesr_amd import tile
    from pesr_amd.model import Generator
    T = _entry("test")
    opt = {"num_channels": 64, "depth": 2, "res_scale": 0.1}
    torch.manual_seed(8)
    G = Generator(dict(opt, wattn_every=1, wattn_dim=64))
    G.load_state_dict(gen_sd(64, 2, 3), strict=False)
    path = str(tmp_path / "wa.pt")
    torch.save(G.state_dict(), path)
    loaded = T.load_generator(opt, path, 4).cuda()
    assert [(k, m.dim, m.shift) for k, m in loaded.wattn.items()] == [("0", 64, 0), ("1", 64, 4)] and T.has_wattn(loaded)
    G.cuda()
    img = detrand.image_batch((1, 3, 13, 9), 81).cuda()           # odd sides: ragged windows on both axes, at both shifts
    with torch.no_grad():
        out, direct = loaded(img), G(img)
        assert out.shape == (1, 3, 52, 36) and bool(torch.isfinite(out).all()) and torch.equal(out, direct)
        ens, ens_direct = T.x8_forward(img, loaded), T.x8_forward(img, G)
        assert ens.shape == (1, 3, 52, 36) and bool(torch.isfinite(ens).all()) and torch.equal(ens, ens_direct)
        # tiled: it runs, and is an approximation (the window grid starts at the tile, not at the image)
        tiled, _ = tile.tiled_forward(loaded, img, 4, 8, 2, 4)
        assert tiled.shape == out.shape and bool(torch.isfinite(tiled).all())
        assert not torch.equal(tiled, out)
