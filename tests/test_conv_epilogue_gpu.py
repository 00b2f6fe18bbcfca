"""GPU: the fused conv epilogue (pesr_amd/csrc/conv_epilogue.h) in EVERY 3x3 conv kernel family, arm by arm:
    y = act(alpha * (conv + bias) [zeroed where mask <= 0] + skip)
Dispatch moves a layer between the families by shape, precision mode and environment switch, so all of them must keep this one
contract; here each family is chosen by the packing handed to ops.conv3x3_fwd / ops.conv3x3_dgrad, at the smallest shapes that
still reach every branch:
  * (2, 7, 12, 64, 128): tiles partly outside the image in every family (the lanes that must not store); W % 4 == 0 for F(4,3),
    Cin % 64 == 0 and Cout % 128 == 0 for F(2,3) and the split-bf16 kernel.  Their input gradient is the conv Cout -> Cin, so its 64
    output channels are no shape of these two kernels (dispatch never gives them one): their input-gradient arms run at
    (2, 7, 12, 128, 128), the smallest Cin they take;
  * (2, 7, 12, 256, 128), the three fp32 families: few tiles and >= 8 chunks of 16 reduction channels, so the kernels split K (direct:
    prep_cfg, 16 tiles of the 768 aimed at, ksplit 4 forward / 2 input gradient; F(2,3): 2 tiles < 160, the same; F(4,3): w4_plan_one,
    the same) and the epilogue runs in the split-K finish kernel;
  * (1, 7, 9, 64, 3) on the direct kernel: an output channel count that is no multiple of 4 takes its scalar epilogue;
  * (1, 13, 11, 64, 128) at stride 2: the bf16 kernel's stride-2 forward and its four-parity-class input gradient.
The expected value composes the operations in that order on the CPU from the oracle's conv (oracle.ops).  Bounds are the project's:
1e-5 of the output's maximum for the fp32 families and split-bf16 against the fp32 oracle, and for bf16 1e-5 against ITS oracle
(both operands rounded to bf16, float64 sums), as tests/test_bf16_gpu.py holds it."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O

pytestmark = pytest.mark.gpu

SLOPE = 0.2
# name -> (bias, alpha, mask, skip, activation)
FWD_ARMS = {
    "plain": (False, 1.0, False, False, "none"),
    "bias": (True, 1.0, False, False, "none"),
    "bias_relu": (True, 1.0, False, False, "relu"),
    "bias_alpha_skip": (True, 0.1, False, True, "none"),
    "bias_mask": (True, 1.0, True, False, "none"),
    "bias_alpha_mask_skip_lrelu": (True, 0.5, True, True, "lrelu"),
}
# name -> (alpha, mask, skip)
DGRAD_ARMS = {"plain": (1.0, False, False), "alpha_mask_skip": (0.5, True, True)}

SMALL, SPLITK, ODD_COUT, STRIDE2 = (2, 7, 12, 64, 128), (2, 7, 12, 256, 128), (1, 7, 9, 64, 3), (1, 13, 11, 64, 128)
# (family, (N, H, W, Cin, Cout), stride)
CASES = [(fam, SMALL, 1) for fam in ("direct", "F(2,3)", "F(4,3)", "bf16", "split-bf16")] + \
        [(fam, SPLITK, 1) for fam in ("direct", "F(2,3)", "F(4,3)")] + \
        [("direct", ODD_COUT, 1), ("bf16", STRIDE2, 2)]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(y):
    return y.permute(0, 3, 1, 2).cpu()


def _close(a, b, rel, what):
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e} > {rel})"


@functools.lru_cache(maxsize=None)
def _problem(shape, stride, bf16):
    """Inputs and the oracle's conv (no bias) / input gradient of one case, computed once and shared by its arms; never modified."""
    N, H, W, Cin, Cout = shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    p = {"x": _rand(N, Cin, H, W, seed=1), "w": _rand(Cout, Cin, 3, 3, seed=2, scale=0.1), "b": _rand(Cout, seed=3),
         "skip": _rand(N, Cout, OH, OW, seed=4), "mask": _rand(N, Cout, OH, OW, seed=5), "dy": _rand(N, Cout, OH, OW, seed=6),
         "dskip": _rand(N, Cin, H, W, seed=7), "dmask": _rand(N, Cin, H, W, seed=8)}
    if bf16:
        p["conv"] = O.conv3x3_bf16(p["x"], p["w"], None, stride)
        xr = O.round_bf16(p["x"]).double().requires_grad_(True)
        F.conv2d(xr, O.round_bf16(p["w"]).double(), None, stride=stride, padding=1).backward(O.round_bf16(p["dy"]).double())
        p["dx"] = xr.grad.float()
    else:
        p["conv"] = O.conv3x3(p["x"], p["w"], None, stride)
        p["dx"] = O.conv3x3_grads(p["x"], p["w"], p["dy"], stride, need_bias=False)[0]
    return p


def _expected_fwd(p, arm):
    bias, alpha, mask, skip, act = FWD_ARMS[arm]
    y = p["conv"] + p["b"].view(1, -1, 1, 1) if bias else p["conv"]
    y = alpha * y
    if mask:
        y = torch.where(p["mask"] > 0, y, torch.zeros_like(y))
    if skip:
        y = y + p["skip"]
    return {"none": y, "relu": torch.relu(y), "lrelu": F.leaky_relu(y, SLOPE)}[act]


def _expected_dgrad(p, arm):
    alpha, mask, skip = DGRAD_ARMS[arm]
    dx = alpha * p["dx"]
    if mask:
        dx = torch.where(p["dmask"] > 0, dx, torch.zeros_like(dx))
    return dx + p["dskip"] if skip else dx


@contextlib.contextmanager
def _mode(fam):
    """The precision mode of the two bf16 families, with the workgroup-count floor lowered as tests/test_bf16_gpu.py does; the C -> 3
    case with ops.USE_RGB_OUT off, so that it is the implicit-GEMM kernel that runs."""
    from pesr_amd import ops
    saved = ops.PRECISION, ops.BF16_MIN_WGS, ops.USE_RGB_OUT
    try:
        if fam in ("bf16", "split-bf16"):
            ops.set_precision(fam)
            ops.BF16_MIN_WGS = 1
        ops.USE_RGB_OUT = False
        yield
    finally:
        ops.PRECISION, ops.BF16_MIN_WGS, ops.USE_RGB_OUT = saved


def run_case(fam, shape, stride):
    """Every arm of one case on the GPU -> [(name, result as NCHW on the CPU, expected)]."""
    from pesr_amd import ops
    pack = {"direct": ops.pack_conv3x3, "F(2,3)": ops.pack_conv3x3_wino, "F(4,3)": ops.pack_conv3x3_wino4, "bf16": ops.pack_conv3x3_bf16,
            "split-bf16": ops.pack_conv3x3_bf16x3}[fam]
    acts = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}
    N, H, W, Cin, Cout = shape
    p = _problem(shape, stride, fam == "bf16")
    out = []
    with _mode(fam):
        x, w, b, skip, mk = _nhwc(p["x"]), p["w"].cuda(), p["b"].cuda(), _nhwc(p["skip"]), _nhwc(p["mask"])
        wf = pack(w, 0)
        for arm, (bias, alpha, mask, skp, act) in FWD_ARMS.items():
            y = ops.conv3x3_fwd(x, wf, b if bias else None, Cout, stride, alpha=alpha, act=acts[act], slope=SLOPE if act == "lrelu" else 0.0,
                                skip=skip if skp else None, mask=mk if mask else None)
            out.append((f"fwd-{arm}", _nchw(y), _expected_fwd(p, arm)))
        if Cout % 16 == 0:          # (the C -> 3 layer's input gradient is another kernel's: conv_rgb_out.hip)
            if fam in ("F(2,3)", "split-bf16") and Cin % 128:      # these kernels' output channels come in 128s
                Cin = 128
                p = _problem((N, H, W, Cin, Cout), stride, False)
            dy, dskip, dmask = _nhwc(p["dy"]), _nhwc(p["dskip"]), _nhwc(p["dmask"])
            wd = pack(p["w"].cuda(), 1)
            for arm, (alpha, mask, skp) in DGRAD_ARMS.items():
                dx = ops.conv3x3_dgrad(dy, wd, (N, H, W, Cin), stride, alpha=alpha, mask=dmask if mask else None, skip=dskip if skp else None)
                out.append((f"dgrad-{arm}", _nchw(dx), _expected_dgrad(p, arm)))
    return out


@pytest.mark.parametrize("fam,shape,stride", CASES, ids=[f"{f}-{'x'.join(map(str, s))}-s{st}" for f, s, st in CASES])
def test_every_epilogue_arm(fam, shape, stride):
    results = run_case(fam, shape, stride)
    assert len(results) == len(FWD_ARMS) + (len(DGRAD_ARMS) if shape[4] % 16 == 0 else 0)
    for name, got, want in results:
        assert got.shape == want.shape, (name, got.shape, want.shape)
        _close(got, want, 1e-5, f"{fam} {shape} stride {stride} {name}")
