"""GPU: the channel attention of the Generator's residual blocks (--attention ca, docs/modes.md section 4u) - its kernels against the
float64 restatement of tests/channel_attention_oracle.py, the autograd node, determinism, ResBlock and Generator against a float64
torch restatement, train steps (eager, captured, resumed, with the moving average) and test.py's loader."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import channel_attention_oracle as O
from helpers import dis_sd, gen_sd, vgg_sd
from oracle import detrand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A32 = float(np.float32(0.1))          # res_scale 0.1 as the C ABI's float carries it
_SHARED = {}


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_cag_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- 1. the two pixel sums ------------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(2, 1, 1, 16), (2, 7, 5, 16), (1, 97, 61, 64), (3, 12, 12, 256)]


@pytest.mark.parametrize("shape", SUM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_and_ds_against_float64_within_the_bound_of_any_summation_order(shape):
    """|err| <= gamma(HW) * (sum |terms|) * scale + one ulp of the result, gamma(n) = n u / (1 - n u), u = 2^-24: the bound of an fp32
    sum of HW terms in ANY order (the kernels add fp32 partials of chunks, the second stage runs in double and rounds once); for ds the
    terms are the exact products gy * t (one fused multiply-add per pixel: the product is never rounded on its own)."""
    from pesr_amd import ops
    N, H, W, C = shape
    if shape == (1, 97, 61, 64):       # several partials and a ragged last one: 46 chunks of 128 pixels and one of 29
        n = ops.ca_pool_partials(N, H * W, C)
        assert n > 2 and (H * W) % n != 0 and (H * W) % 128 == 29 and n == -(-(H * W) // 128)
    elif shape == (3, 12, 12, 256):
        assert ops.ca_pool_partials(N, H * W, C) > 1
    t, gy = O.features(shape, 11), O.features(shape, 12, scale=1e-3, offset=1e-4)
    m = ops.ca_pool(_cuda(t)).cpu().double()
    want = O.pool(t)
    bound = O.sum_bound(t, 1.0 / (H * W), want)
    err = (m - want).abs()
    print(f"pool {shape}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    ds = ops.ca_ds(_cuda(gy), _cuda(t), A32).cpu().double()
    terms = O._t(gy) * O._t(t)
    want = O.ds_sum(gy, t, A32)
    bound = O.sum_bound(terms, A32, want)
    err = (ds - want).abs()
    print(f"ds   {shape}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ---- 2. the gate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, C, reduction", [(2, 16, 16), (2, 16, 4), (3, 256, 16), (1, 64, 8)])
def test_gate_forward_and_backward_against_float64(N, C, reduction):
    from pesr_amd import ops
    c = O.gate_case(N, C, reduction, 21)
    d = {k: _cuda(v) for k, v in c.items()}
    ref = O.gate(c["m"], c["w1"], c["b1"], c["w2"], c["b2"])
    assert float(ref["h"][0, 0]) == 0.0 and float(ref["z1"][0, 0]) < -0.5            # a shut ReLU
    assert abs(float(ref["z2"][0, 0]) - 20.0) < 1e-12 and abs(float(ref["z2"][0, 1]) + 20.0) < 1e-12      # saturated sigmoids
    h, s = ops.ca_gate_fwd(d["m"], d["w1"], d["b1"], d["w2"], d["b2"])
    assert h.shape == (N, C // reduction) and s.shape == (N, C)
    assert O.rel_err(h, ref["h"]) <= 1e-4 and O.rel_err(s, ref["s"]) <= 1e-4
    assert bool(((h.cpu() == 0) == (ref["h"] == 0)).all())                           # the same ReLUs are open
    assert float(h[0, 0]) == 0.0
    got = ops.ca_gate_bwd(d["ds"], s, h, d["m"], d["w1"], d["w2"])
    want = O.gate_backward(c["ds"], ref["s"], ref["h"], c["m"], c["w1"], c["w2"])
    for name, g in zip(("dm", "dw1", "db1", "dw2", "db2"), got):
        assert g.numel() == want[name].numel()
        e = O.rel_err(g, want[name])
        print(f"gate ({N},{C},{reduction}) {name}: {e:.2e}")
        assert e <= 1e-4, (name, e)
    # the 1 x 1 convs' own shapes go in and come out as they are
    w1c, w2c = d["w1"].reshape(-1, C, 1, 1), d["w2"].reshape(C, -1, 1, 1)
    got4 = ops.ca_gate_bwd(d["ds"], s, h, d["m"], w1c, w2c)
    assert got4[1].shape == w1c.shape and got4[3].shape == w2c.shape
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got, got4))


# ---- 3. / 4. the node -----------------------------------------------------------------------------------------------------------------
NODE_CASES = [((2, 7, 5, 16), 4, 0.1), ((2, 7, 5, 16), 4, 1.0), ((2, 12, 12, 64), 16, 0.1), ((2, 12, 12, 64), 16, 1.0)]


def _node_inputs(shape, reduction):
    key = ("node", shape, reduction)
    if key not in _SHARED:
        C = shape[-1]
        R = C // reduction
        g = np.random.default_rng(31)
        w = dict(w1=(g.standard_normal((R, C, 1, 1)) / np.sqrt(C)).astype(np.float32), b1=(g.standard_normal(R) * 0.1).astype(np.float32),
                 w2=(g.standard_normal((C, R, 1, 1)) / np.sqrt(R)).astype(np.float32), b2=(g.standard_normal(C) * 0.1).astype(np.float32))
        _SHARED[key] = dict(x=O.features(shape, 32), t=O.features(shape, 33), gy=O.features(shape, 34, scale=1e-2, offset=1e-3), **w)
    return _SHARED[key]


def _node_reference(shape, reduction, a):
    key = ("node-ref", shape, reduction, a)
    if key not in _SHARED:
        c = _node_inputs(shape, reduction)
        z1 = O.gate(O.pool(c["t"]), c["w1"], c["b1"], c["w2"], c["b2"])["z1"]
        assert float(z1.abs().min()) > 1e-4          # fp32 and float64 agree on which ReLUs are open
        _SHARED[key] = O.node_grads(c["x"], c["t"], c["w1"], c["b1"], c["w2"], c["b2"], a, c["gy"])
    return _SHARED[key]


def _run_node(shape, reduction, a):
    from pesr_amd import functional as PF
    c = _node_inputs(shape, reduction)
    leaves = [_cuda(c[k]).requires_grad_(True) for k in ("x", "t", "w1", "b1", "w2", "b2")]
    gy = _cuda(c["gy"])
    y = PF.ChannelAttentionFn.apply(*leaves, a)
    y.backward(gy)
    return y.detach(), [v.grad for v in leaves], gy


@pytest.mark.parametrize("shape, reduction, a", NODE_CASES)
def test_node_forward_and_six_gradients_against_float64_autograd(shape, reduction, a):
    y, grads, gy = _run_node(shape, reduction, a)
    y64, g64 = _node_reference(shape, reduction, a)
    err = (y.cpu().double() - y64).abs()
    assert bool((err <= 1e-5 * y64.abs() + 1e-5 * float(y64.abs().max())).all()), float(err.max())
    assert torch.equal(grads[0], gy)                 # gx is gy bit for bit
    for name, g, w in zip(("gx", "gt", "gw1", "gb1", "gw2", "gb2"), grads, g64):
        assert g.shape == w.shape
        e = O.rel_err(g, w)
        print(f"node {shape} a={a} {name}: {e:.2e}")
        assert e <= 1e-4, (name, e)


@pytest.mark.parametrize("shape, reduction, a", NODE_CASES[1:3])
def test_node_is_deterministic_and_fp32_in_every_precision_mode(shape, reduction, a):
    from pesr_amd import ops
    first = _run_node(shape, reduction, a)
    second = _run_node(shape, reduction, a)
    before = ops.PRECISION
    ops.set_precision("bf16")
    try:
        third = _run_node(shape, reduction, a)
    finally:
        ops.set_precision(before)
    fourth = _run_node(shape, reduction, a)
    for other in (second, third, fourth):
        assert torch.equal(first[0], other[0])
        for g0, g1 in zip(first[1], other[1]):
            assert torch.equal(g0, g1)


# ---- 5. ResBlock and Generator --------------------------------------------------------------------------------------------------------
def _module_vs_float64(module, x, forward64, atol, what):
    """module (on the GPU) on x [N, C, H, W] float32 numpy against forward64(float64 leaves of its state_dict, x): the output within atol
    + 1e-5 |ref|, every parameter gradient of an L1 loss against a fixed seeded target within 1e-4 of its tensor's maximum."""
    xg = _cuda(x).contiguous(memory_format=torch.channels_last)
    y = module(xg)
    sd = O.double_leaves(module.state_dict())
    y64 = forward64(sd, torch.as_tensor(x).double())
    err = (y.detach().cpu().double() - y64.detach()).abs()
    assert bool((err <= atol + 1e-5 * y64.detach().abs()).all()), (what, float(err.max()))
    target = torch.as_tensor(O.features(tuple(y64.shape), 55, scale=float(y64.detach().abs().mean()), offset=0.0))
    (y - target.cuda()).abs().mean().backward()
    (y64 - target.double()).abs().mean().backward()
    for k, p in module.named_parameters():
        assert p.grad is not None and sd[k].grad is not None and float(sd[k].grad.abs().max()) > 0, k
        e = O.rel_err(p.grad, sd[k].grad)
        print(f"{what} {k}: {e:.2e}")
        assert e <= 1e-4, (what, k, e)


@pytest.mark.parametrize("bias", [True, False], ids=["fused", "unfused-no-bias"])
def test_resblock_against_float64(bias):
    from pesr_amd.model.basic import ResBlock
    torch.manual_seed(9)          # (a seed under which, for both variants, some of the gate's hidden units are open and some shut)
    blk = ResBlock(16, 3, bias=bias, res_scale=0.1, attention="ca", reduction=4).cuda()
    assert blk._fused == bias and [k for k in blk.state_dict() if k.startswith("ca.")] == [
        "ca.squeeze.weight", "ca.squeeze.bias", "ca.excite.weight", "ca.excite.bias"]
    x = np.ascontiguousarray(O.features((2, 12, 12, 16), 51, scale=40.0, offset=10.0).transpose(0, 3, 1, 2))
    _module_vs_float64(blk, x, lambda sd, x64: O.resblock(sd, x64, 0.1), 2e-3, "ResBlock" + ("" if bias else "(bias=False)"))


def test_generator_against_float64():
    from pesr_amd.model import Generator
    torch.manual_seed(6)
    G = Generator({"num_channels": 16, "depth": 2, "res_scale": 0.1, "attention": "ca", "ca_reduction": 4})
    G.load_state_dict(gen_sd(16, 2, 0), strict=False)        # seeded conv weights; the attention keeps its own seeded initialisation
    G.cuda()
    x = detrand.image_batch((2, 3, 12, 12), 61).numpy().astype(np.float32)
    assert x.min() >= 0 and x.max() <= 255 and np.array_equal(x, np.round(x))
    _module_vs_float64(G, x, lambda sd, x64: O.generator(sd, x64, 2, 0.1), 2e-3, "Generator")


# ---- 6. / 7. train steps --------------------------------------------------------------------------------------------------------------
CH, DEPTH, PS, BATCH, LR, RED = 64, 2, 8, 2, 5e-5, 16
G_OPT = {"num_channels": CH, "depth": DEPTH, "res_scale": 0.1, "scale": 4, "attention": "ca", "ca_reduction": RED}


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
def test_eager_steps_are_finite_and_move_the_attention(phase):
    logs, states, start, end = _four_eager(phase)
    assert all(np.isfinite(v) for l in logs[:2] for v in l.values()), logs[:2]
    ca = [k for k in start if ".ca." in k]
    assert len(ca) == 4 * DEPTH
    for k in ca:
        assert not torch.equal(start[k], end[k]), k
        assert bool(torch.isfinite(end[k]).all()), k


def test_discriminator_step_is_the_same_bits_for_the_same_generator():
    """Attention changes nothing in D's code: a second run from the same weights leaves D's parameters and BatchNorm statistics after
    the first step's D phase bit for bit (D's step reads G's output before G moves)."""
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


def test_moving_average_generator_has_attention_of_its_own():
    from pesr_amd.model.basic import ChannelAttention
    tr = _trainer("pretrain", ema_decay=0.9)
    G_ema = tr.optim_G.ema_module(tr.G)
    assert [m.reduction for m in G_ema.modules() if isinstance(m, ChannelAttention)] == [RED] * DEPTH
    for lr, hr in _data()[:2]:
        tr.pretrain_step(lr, hr)
    tr.optim_G.refresh_ema()
    live, ema = dict(tr.G.named_parameters()), dict(G_ema.named_parameters())
    ca = [k for k in live if ".ca." in k]
    assert len(ca) == 4 * DEPTH
    for k in ca:
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
    assert any(".ca." in k for k in st["G"])
    fresh = _trainer("train", seed=40)              # other weights, zero moments
    assert not torch.equal(fresh.optim_G.flat.flat_p, states4[1]["G"])
    fresh.G.load_state_dict(st["G"]); fresh.D.load_state_dict(st["D"])
    fresh.optim_G.load_state_dict(st["optim_G"]); fresh.optim_D.load_state_dict(st["optim_D"])
    for i in (2, 3):
        assert _logs(fresh.gan_step(*data[i])) == logs4[i], i
        _assert_state(fresh, states4[i], f"resumed, step {i + 1}")


# ---- 8. inference plumbing ------------------------------------------------------------------------------------------------------------
def test_loader_of_test_py_runs_an_odd_single_image_and_the_ensemble(tmp_path):
    from pesr_amd.model import Generator
    from pesr_amd.model.basic import ChannelAttention
    T = _entry("test")
    opt = {"num_channels": 16, "depth": 2, "res_scale": 0.1}
    torch.manual_seed(8)
    G = Generator(dict(opt, attention="ca", ca_reduction=4))
    G.load_state_dict(gen_sd(16, 2, 3), strict=False)
    path = str(tmp_path / "ca.pt")
    torch.save(G.state_dict(), path)
    loaded = T.load_generator(opt, path, 4).cuda()
    assert [m.reduction for m in loaded.modules() if isinstance(m, ChannelAttention)] == [4, 4] and T.has_attention(loaded)
    G.cuda()
    img = detrand.image_batch((1, 3, 13, 9), 81).cuda()           # odd sides, N = 1: the single-image chunking of the pool
    with torch.no_grad():
        out, direct = loaded(img), G(img)
        assert out.shape == (1, 3, 52, 36) and bool(torch.isfinite(out).all()) and torch.equal(out, direct)
        ens, ens_direct = T.x8_forward(img, loaded), T.x8_forward(img, G)
        assert ens.shape == (1, 3, 52, 36) and torch.equal(ens, ens_direct)
        assert float((ens - out).abs().max()) > 0             # the gate is not equivariant bit for bit, the ensemble is another image
