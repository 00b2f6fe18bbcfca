"""GPU: the F(4,3) kernel (conv3x3_wino4.hip) in both forms of its last chunk, against each other and against the oracle: the TAIL form -
the last chunk run group-major, each group of three m-tiles transformed, exchanged and stored under the MFMAs of the groups behind it - and
the form without it (PESR_WINO4_TAIL=0), which is also what split-K, the dense layout, BatchNorm and multi-round launches run.

Every case runs the kernel through the C ABI twice, with PESR_WINO4_TAIL unset and set to 0: the two results are the same bits
(torch.equal: same products, same order of additions), and each is within 1e-5 of the oracle's maximum - the bound tests/test_conv_gpu.py
holds this kernel to.  The shapes are the smallest that reach the chunk loop's edges: one chunk (the loop body not at all: weight slabs 0
and 1 from the prologue), two and three chunks (the body once, twice in front of the peeled chunk), 24-x-tile rows, tile rows past the
image (masked stores in every group), several tiles with two n-tiles; with bias + ReLU, skip with alpha, mask, and the fused PixelShuffle
on either side.  Rows of 8 and 16 x-tiles (row length at run time) with and without a ragged edge, the dense layout, split-K, stacked
images and the BatchNorm epilogue in both modes (all four of its instantiations) never take the TAIL form: they must run the kernel
they ran before and agree all the same.  A launch refuses BatchNorm sums whose rows are not the rows of `part`."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import close
from oracle import ops as O

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(y):
    return y.permute(0, 3, 1, 2).cpu()


def _both(monkeypatch, run):
    """run() with the TAIL form and under PESR_WINO4_TAIL=0 -> both results, after torch.equal of every tensor of the two"""
    monkeypatch.delenv("PESR_WINO4_TAIL", raising=False)
    new = run()
    monkeypatch.setenv("PESR_WINO4_TAIL", "0")
    assert os.environ["PESR_WINO4_TAIL"] == "0"
    old = run()
    monkeypatch.delenv("PESR_WINO4_TAIL")
    torch.cuda.synchronize()
    for a, b in zip(new if isinstance(new, tuple) else (new,), old if isinstance(old, tuple) else (old,)):
        assert a.shape == b.shape and torch.equal(a, b), "the two forms must give the same bits"
    return new, old


# N, H, W, Cin, Cout
TAIL_SHAPES = [
    (1, 12, 48, 16, 64),      # one chunk: slabs 0, 1 from the prologue
    (1, 12, 48, 32, 64),      # two chunks
    (1, 12, 48, 48, 64),      # three
    (1, 6, 96, 48, 64),       # 24-x-tile rows
    (1, 8, 48, 32, 64),       # tile rows past the image: masked stores in every group
    (3, 12, 48, 32, 128),     # several tiles and two n-tiles
]
FALLBACK_SHAPES = [
    (1, 12, 24, 32, 64),      # rows of 8 x-tiles (the row length at run time), six of them and 12 of the 18 tile rows inside the image
    (1, 12, 20, 48, 64),      # the same with a ragged edge: five x-tiles
    (2, 12, 12, 512, 512),    # split-K
    (16, 12, 12, 512, 512),   # stacked images (and split-K), in the dense layout: rows of 3 x-tiles
    (1, 18, 32, 32, 64),      # rows of 8 x-tiles, the 18 x 8 tile full
    (1, 9, 64, 32, 64),       # rows of 16 x-tiles
    (1, 16, 36, 32, 64),      # dense layout: rows of 9 x-tiles
]


@pytest.mark.parametrize("N,H,W,Cin,Cout", TAIL_SHAPES + FALLBACK_SHAPES)
def test_forms_of_the_epilogue(monkeypatch, N, H, W, Cin, Cout):
    from pesr_amd import ops
    x = _rand(N, Cin, H, W, seed=1); w = _rand(Cout, Cin, 3, 3, seed=2, scale=0.1); b = _rand(Cout, seed=3)
    skip = _rand(N, Cout, H, W, seed=4); mk = _rand(N, Cout, H, W, seed=5)
    ref = O.conv3x3(x, w, b)
    xg, bg, sg, mg = _nhwc(x), b.cuda(), _nhwc(skip), _nhwc(mk)
    wf = ops.pack_conv3x3_wino4(w.cuda(), 0)
    want = {"bias + ReLU": torch.relu(ref), "skip": ref * 0.1 + skip, "mask": torch.where(mk > 0, ref, torch.zeros_like(ref))}
    runs = {"bias + ReLU": lambda: ops.conv3x3_fwd(xg, wf, bg, Cout, act=ops.ACT_RELU),
            "skip": lambda: ops.conv3x3_fwd(xg, wf, bg, Cout, alpha=0.1, skip=sg),
            "mask": lambda: ops.conv3x3_fwd(xg, wf, bg, Cout, mask=mg)}
    for form, run in runs.items():
        new, old = _both(monkeypatch, run)
        close(_nchw(new), want[form], TOL, what=f"{form}, TAIL")
        close(_nchw(old), want[form], TOL, what=f"{form}, PESR_WINO4_TAIL=0")


@pytest.mark.parametrize("Cin", [16, 32, 48])
def test_pixel_shuffle_on_either_side(monkeypatch, Cin):
    from pesr_amd import ops
    N, H, W, C = 1, 12, 48, 64
    x = _rand(N, Cin, H, W, seed=1); w = _rand(4 * C, Cin, 3, 3, seed=2, scale=0.1); b = _rand(4 * C, seed=3)
    ref = F.pixel_shuffle(O.conv3x3(x, w, b), 2)
    xg = _nhwc(x); wf = ops.pack_conv3x3_wino4(w.cuda(), 0, ps=True); bp = ops.pack_bias_ps(b.cuda())
    new, old = _both(monkeypatch, lambda: ops.conv3x3_fwd(xg, wf, bp, 4 * C, ps_out=True))
    close(_nchw(new), ref, TOL, what="ps, TAIL"); close(_nchw(old), ref, TOL, what="ps, PESR_WINO4_TAIL=0")
    # the input gradient of a C -> 4 C conv reads the shuffled gradient: 4 C input channels of the kernel, C = 64 out
    xi = _rand(N, C, H, W, seed=6); wi = _rand(4 * C, C, 3, 3, seed=7, scale=0.1); dys = _rand(N, C, 2 * H, 2 * W, seed=8)
    dx_ref, _, _ = O.conv3x3_grads(xi, wi, F.pixel_unshuffle(dys, 2))
    dg = _nhwc(dys); wd = ops.pack_conv3x3_wino4(wi.cuda(), 1, ps=True)
    new, old = _both(monkeypatch, lambda: ops.conv3x3_dgrad(dg, wd, (N, H, W, C), ps_in=True))
    close(_nchw(new), dx_ref, TOL, what="ps_in, TAIL"); close(_nchw(old), dx_ref, TOL, what="ps_in, PESR_WINO4_TAIL=0")


# H, W, Cin: rows of 12 x-tiles with one, two and three chunks; of 24; of 8 (row length at run time: tile partly, then wholly inside the
# image); the dense layout (rows of 9)
BN_SHAPES = [(12, 48, 16), (12, 48, 32), (12, 48, 48), (6, 96, 32), (12, 24, 32), (18, 32, 32), (16, 36, 32)]


@pytest.mark.parametrize("H,W,Cin", BN_SHAPES)
def test_batchnorm_epilogue_both_modes(monkeypatch, H, W, Cin):
    from pesr_amd import ops
    N, C = 1, 64
    # mode 1: z = conv(x) and the sums of z, z^2 per pixel tile
    x = _rand(N, Cin, H, W, seed=1); w = _rand(C, Cin, 3, 3, seed=2, scale=0.1)
    xg = _nhwc(x); wf = ops.pack_conv3x3_wino4(w.cuda(), 0)
    assert ops.conv_bn_rows(2, N, H, W, Cin, C, 1) > 0
    (z, part), (z0, part0) = _both(monkeypatch, lambda: ops.conv3x3_fwd_bn_stats(xg, wf, None, C, 1))
    ref = O.conv3x3(x, w, None)
    close(_nchw(z), ref, TOL, what="z, TAIL"); close(_nchw(z0), ref, TOL, what="z, PESR_WINO4_TAIL=0")
    close(part[:, 0].sum(0), ref.double().sum((0, 2, 3)), TOL, atol=TOL * ref.abs().sum((0, 2, 3)).max().item(), what="sum z")
    # mode 2: the input gradient of the next conv (Cin channels out of it), times lrelu'(bn(z)), and its sums
    zc = _rand(N, C, H, W, seed=3, scale=2.0); gamma = _rand(C, seed=4) * 0.5 + 1.0; beta = _rand(C, seed=5, scale=0.3)
    wn = _rand(Cin, C, 3, 3, seed=6, scale=0.1); dy = _rand(N, Cin, H, W, seed=7)
    zg, dyg = _nhwc(zc), _nhwc(dy)
    _, stats = ops.bn_lrelu_fwd(zg, gamma.cuda(), beta.cuda(), torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros((), dtype=torch.long).cuda())
    wd = ops.pack_conv3x3_wino4(wn.cuda(), 1)
    (gm, p2), (gm0, p20) = _both(monkeypatch, lambda: ops.conv3x3_dgrad_bn_sums(dyg, wd, tuple(zg.shape), 1, zg, stats, gamma.cuda(), beta.cuda(), 0.2))
    dx_ref, _, _ = O.conv3x3_grads(zc, wn, dy)
    st = stats.cpu()
    zz = gamma[None, :, None, None] * ((zc - st[0][None, :, None, None]) * st[1][None, :, None, None]) + beta[None, :, None, None]
    far = (zz.abs() > 1e-5).float()                       # at the kink the sign of bn(z) is a matter of rounding
    want = torch.where(zz > 0, dx_ref, 0.2 * dx_ref) * far
    close(_nchw(gm) * far, want, TOL, what="g', TAIL"); close(_nchw(gm0) * far, want, TOL, what="g', PESR_WINO4_TAIL=0")


def test_bn_rows_must_equal_the_rows_of_part():
    from pesr_amd import _lib, ops
    import ctypes
    N, H, W, Cin, C = 1, 12, 48, 32, 64
    xg = _nhwc(_rand(N, Cin, H, W, seed=1)); wf = ops.pack_conv3x3_wino4(_rand(C, Cin, 3, 3, seed=2, scale=0.1).cuda(), 0)
    rows = ops.conv_bn_rows(2, N, H, W, Cin, C, 1)
    assert rows > 0
    y = torch.empty((N, H, W, C), device="cuda")
    L = _lib.lib()
    for r, want in ((rows, 0), (rows + 1, -1), (rows + 7, -1)):        # -1: PESR_EINVAL
        part = torch.zeros((r, 2, C), device="cuda")
        f = ops._fuse_struct(ops.BN_FWD_STATS, part)
        rc = L.pesr_conv3x3_wino4_bn(ops._p(xg), ops._p(wf.t), None, ops._p(y), N, H, W, Cin, C, None, 0, ctypes.byref(f), ops._stream())
        assert rc == want, (r, rows, rc)
    # the direct kernel's twin
    wp = ops.pack_conv3x3(_rand(C, Cin, 3, 3, seed=2, scale=0.1).cuda(), 0)
    rows = ops.conv_bn_rows(0, N, H, W, Cin, C, 1)
    assert rows > 0
    nws = L.pesr_conv3x3_workspace_bytes(N, H, W, C)
    ws = ops.workspace(nws, xg.device) if nws else None
    for r, want in ((rows, 0), (rows + 1, -1)):
        part = torch.zeros((r, 2, C), device="cuda")
        f = ops._fuse_struct(ops.BN_FWD_STATS, part)
        rc = L.pesr_conv3x3_fwd_bn(ops._p(xg), ops._p(wp), None, ops._p(y), N, H, W, Cin, C, 1, ops._p(ws), nws, ctypes.byref(f), ops._stream())
        assert rc == want, (r, rows, rc)
    torch.cuda.synchronize()
