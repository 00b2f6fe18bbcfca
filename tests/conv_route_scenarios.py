"""The scenarios whose kernel launches tests/golden/conv_route_trace.json pins (tests/test_conv_route_gpu.py replays them,
tests/golden/make_golden_conv_route.py recorded them) and the shim that records a launch trace.

A launch entry point is a function of pesr_amd._lib.SIGNATURES whose last argument is the stream.  Per launch the trace keeps the name,
every c_int / c_long / c_float argument, "p" / "0" for a non-null / null pointer and "current" / "side" for the stream.  c_size_t
arguments (workspace sizes grow with what ran before) and the memoised host-only queries (planners, scores, rows, workspace bytes) are
not part of it.  Every scenario builds its modules afresh and returns the tensors it computed: {name: tensor}.
"""
import contextlib
from ctypes import c_size_t, c_void_p

import torch

from helpers import gen_sd
from oracle import detrand
from test_model_gpu import _trainer

BODY_X = (16, 256, 48, 48)          # the body shape of tests/test_fullsize_gpu.py: the F(4,3) planner refuses what does not fill the chip


def _is_launch(name, sig):
    res, args = sig
    return bool(args) and args[-1] is c_void_p and not name.startswith("pesr_peer_")


@contextlib.contextmanager
def recording(trace):
    """Every launch through pesr_amd._lib.lib() inside the block is appended to `trace` (ctypes function objects cannot be
    monkeypatched in place: the library handle is wrapped, as tests/test_fullsize_gpu.py does)."""
    from pesr_amd import _lib
    from pesr_amd import functional as PF
    L = _lib.lib()
    real_lib = _lib.lib
    wrapped = {}

    def wrap(name):
        fn = getattr(L, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None or not _is_launch(name, sig):
            return fn
        types = sig[1]

        def f(*args):
            row = [name]
            for a, t in zip(args[:-1], types[:-1]):
                if t is c_size_t:
                    continue
                if t is c_void_p:
                    row.append("p" if a is not None and a != 0 else "0")
                else:
                    row.append(a if isinstance(a, (int, float)) else a.value)
            side = {s.cuda_stream for s in PF._SIDE.values()}
            row.append("side" if args[-1] in side else "current")
            trace.append(row)
            return fn(*args)
        return f

    class _Shim:
        def __getattr__(self, name):
            f = wrapped.get(name)
            if f is None:
                f = wrapped[name] = wrap(name)
            return f
    shim = _Shim()
    _lib.lib = lambda: shim
    try:
        yield trace
    finally:
        _lib.lib = real_lib


@contextlib.contextmanager
def _set(obj, **kw):
    saved = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def _precision(p):
    from pesr_amd import ops
    saved = ops.PRECISION
    ops.set_precision(p)
    try:
        yield
    finally:
        ops.set_precision(saved)


def _state(out, G, D):
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v
        for k, p in net.named_parameters():
            if p.grad is not None:
                out[f"{tag}.grad.{k}"] = p.grad
    return out


def trainer_steps():
    """One pretrain step and two GAN steps of the 16-channel networks: first and second use of the Discriminator's blocks, the
    BatchNorm links, the VGG tail, the RGB layers in both directions."""
    tr, G, D = _trainer(16, 2, 8)
    out = {}
    lr, hr = detrand.image_batch((4, 3, 8, 8), 100).cuda(), detrand.image_batch((4, 3, 32, 32), 200).cuda()
    out["pretrain.l1"] = torch.as_tensor(float(tr.pretrain_step(lr, hr)["l1"]))
    for it in range(2):
        lr, hr = detrand.image_batch((4, 3, 8, 8), 100 + it).cuda(), detrand.image_batch((4, 3, 32, 32), 200 + it).cuda()
        log = tr.gan_step(lr, hr)
        out[f"gan{it}.losses"] = torch.tensor([float(log[k]) for k in ("l1", "vgg", "g", "tv", "d")], dtype=torch.float64)
    return _state(out, G, D)


def penalty_step():
    """The step of test_gv11_gradient_penalty_step_vs_reference: Conv2Fn and its twice-differentiable companions."""
    tr, G, D = _trainer(16, 2, 8)
    tr.gradient_penalty = True
    lr, hr = detrand.image_batch((4, 3, 8, 8), 100).cuda(), detrand.image_batch((4, 3, 32, 32), 200).cuda()
    u = detrand.uniform((4, 1, 1, 1), 77, 0.0, 1.0).cuda()
    log = tr.gan_step(lr, hr, gp_u=u)
    out = {"losses": torch.tensor([float(log[k]) for k in ("gp", "d")], dtype=torch.float64)}
    return _state(out, G, D)


_BIG = {}


def _big(shape, seed):
    """Deterministic values in [-1, 1) made on the device (a multiplicative hash of the index), built once and shared: the oracle's
    host generator takes seconds at the body shape."""
    t = _BIG.get((shape, seed))
    if t is None:
        n = 1
        for d in shape:
            n *= d
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        h = ((i + seed * 7919) * 2654435761) & 0xFFFFFFFF
        h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
        t = _BIG[(shape, seed)] = ((h >> 8).double() / float(1 << 23) - 1.0).float().reshape(shape)
    return t


def _fwd_bwd(blk, x, gy):
    blk = blk.cuda()
    xg = x.cuda().clone().requires_grad_(True)
    y = blk(xg)
    y.backward(gy.cuda())
    out = {"y": y.detach(), "dx": xg.grad}
    for k, p in blk.named_parameters():
        if p.grad is not None:
            out["grad." + k] = p.grad
    for k, b in blk.named_buffers():
        out["buf." + k] = b
    return out


BASIC_ROWS = [(True, True, "relu", True), (False, True, "lrelu", False), (True, False, "lrelu", True),
              (False, True, None, True), (True, True, "lrelu", False), (False, False, "relu", True)]
RES_ROWS = [(True, True, "relu"), (False, False, "relu"), (True, False, "lrelu")]


def basic_block(bias, bn, act, train):
    """A parameter row of test_basic_block_constructor_branches, at its shapes."""
    import torch.nn as nn
    from model import BasicBlock
    torch.manual_seed(3)
    blk = BasicBlock(32, 64, 3, stride=1, bias=bias, bn=bn, sn=False,
                     act={"relu": nn.ReLU(True), "lrelu": nn.LeakyReLU(0.2, True), None: None}[act])
    if bn:
        with torch.no_grad():
            m = blk[1]
            m.running_mean.copy_(detrand.uniform((64,), 5, -0.2, 0.2)); m.running_var.copy_(detrand.uniform((64,), 6, 0.5, 1.5))
            m.weight.copy_(detrand.uniform((64,), 7, 0.5, 1.5)); m.bias.copy_(detrand.uniform((64,), 8, -0.1, 0.1))
    blk.train(train)
    return _fwd_bwd(blk, detrand.uniform((2, 32, 12, 16), 11), detrand.uniform((2, 64, 12, 16), 12))


def res_block(bias, bn, act):
    """A parameter row of test_res_block_constructor_branches, at its shapes."""
    import torch.nn as nn
    from model import ResBlock
    torch.manual_seed(4)
    blk = ResBlock(64, 3, bias=bias, bn=bn, act=nn.ReLU(True) if act == "relu" else nn.LeakyReLU(0.1, True), res_scale=0.3)
    return _fwd_bwd(blk, detrand.uniform((2, 64, 10, 12), 21), detrand.uniform((2, 64, 10, 12), 22))


def body_res_block():
    from model import ResBlock
    torch.manual_seed(6)
    return _fwd_bwd(ResBlock(256, 3, res_scale=0.1), _big(BODY_X, 41), _big(BODY_X, 42))


def body_ps_conv():
    """Conv(256, 1024, 3) with the PixelShuffle fused into its store (the Upsampler's first conv)."""
    from model import Conv
    from pesr_amd import functional as PF
    torch.manual_seed(7)
    conv = Conv(256, 1024, 3)
    conv.packed = PF.PackedConvWeights(ps=True)
    return _fwd_bwd(conv, _big(BODY_X, 43), _big((16, 256, 96, 96), 44))


def small_generator():
    """Forward and backward of the 16-channel Generator: every node of the Generator, each used once."""
    from model import Generator
    G = Generator({"num_channels": 16, "depth": 2, "res_scale": 0.1}); G.load_state_dict(gen_sd(16, 2))
    return _fwd_bwd(G, detrand.image_batch((4, 3, 8, 8), 100), detrand.uniform((4, 3, 32, 32), 45))


def _switches():
    from pesr_amd import ops
    return [("default", lambda: contextlib.nullcontext()),
            ("USE_WINO4=0", lambda: _set(ops, USE_WINO4=False)),
            ("USE_WINO=USE_WGRAD_WINO=0", lambda: _set(ops, USE_WINO=False, USE_WGRAD_WINO=False)),
            ("bf16", lambda: _precision("bf16")),
            ("split-bf16", lambda: _precision("split-bf16"))]


def scenarios():
    """[(name, context factory, function)]: run `function()` inside `context()`."""
    from pesr_amd import functional as PF
    none = contextlib.nullcontext
    sc = [("trainer", none, trainer_steps), ("penalty", none, penalty_step)]
    sc += [(f"basic_block[{'-'.join(map(str, r))}]", none, (lambda r=r: basic_block(*r))) for r in BASIC_ROWS]
    sc += [(f"res_block[{'-'.join(map(str, r))}]", none, (lambda r=r: res_block(*r))) for r in RES_ROWS]
    for sw, ctx in _switches():
        sc += [(f"body_res_block[{sw}]", ctx, body_res_block), (f"body_ps_conv[{sw}]", ctx, body_ps_conv)]
    # the side stream for every node that has one (each layer used once: the in-place second use of a parameter assumes one stream)
    side = lambda: _set(PF, SIDE_MODE="1")
    sc += [("side:body_res_block", side, body_res_block), ("side:body_ps_conv", side, body_ps_conv), ("side:generator", side, small_generator)]
    sc += [(f"side:basic_block[{'-'.join(map(str, r))}]", side, (lambda r=r: basic_block(*r))) for r in BASIC_ROWS]
    sc += [(f"side:res_block[{'-'.join(map(str, r))}]", side, (lambda r=r: res_block(*r))) for r in RES_ROWS]
    return sc


def run(name_ctx_fn):
    """-> (trace, tensors) of one scenario."""
    name, ctx, fn = name_ctx_fn
    trace = []
    with ctx(), recording(trace):
        out = fn()
    torch.cuda.synchronize()
    return trace, out


def pack_traces(traces):
    """{scenario: [row]} -> {"calls": [distinct row], "scenarios": {scenario: [index into calls]}} (each distinct call kept once)."""
    calls, index, packed = [], {}, {}
    for name, rows in traces.items():
        ids = []
        for r in rows:
            k = repr(r)
            if k not in index:
                index[k] = len(calls)
                calls.append(r)
            ids.append(index[k])
        packed[name] = ids
    return {"calls": calls, "scenarios": packed}
