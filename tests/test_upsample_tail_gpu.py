"""GPU: the backward of the upsampler's tail (conv C -> 4C, PixelShuffle(2), conv C -> 3) run as the backward of one virtual
3x3 conv from C to 64 channels (csrc/upsample_tail.hip, functional.UpsampleTailFn; docs/experiments/upsample_tail.md).

The references are float64 restatements on the CPU: torch indexing for the gather, einsums over the explicit matrix A for the
compose and chain sums, torch autograd of conv -> pixel_shuffle -> conv for the whole pair."""
import pytest
import torch
import torch.nn.functional as F

from helpers import adam_close, close, gen_sd
from oracle import detrand

pytestmark = pytest.mark.gpu


def _rand(gen, *shape, scale=1.0):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * scale


def _A(w4):
    """A [4C, 48] in float64: A[4c+2i+j, (k*4+p)*4+q] = W4[k, c, i+2-p, j+2-q] where both taps lie in 0..2, else 0."""
    C = w4.shape[1]
    A = torch.zeros(4 * C, 48, dtype=torch.float64)
    rows = 4 * torch.arange(C)
    for i in range(2):
        for j in range(2):
            for k in range(3):
                for p in range(4):
                    for q in range(4):
                        a, b = i + 2 - p, j + 2 - q
                        if 0 <= a <= 2 and 0 <= b <= 2:
                            A[rows + 2 * i + j, (k * 4 + p) * 4 + q] = w4[k, :, a, b].double()
    return A


def _chain_ref(w2, b2, w4, S, T):
    """(dW2, db2, dW4, db4) in float64 from the virtual conv's weight gradient S [64, C, 3, 3] and bias gradient T [64]."""
    C = w4.shape[1]
    A, S48, T48 = _A(w4), S[:48].double(), T[:48].double()
    dw2 = torch.einsum("mz,zcef->mcef", A, S48)
    db2 = A @ T48
    R = torch.einsum("mcef,zcef->mz", w2.double(), S48) + torch.outer(b2.double(), T48)
    dw4 = torch.zeros(3, C, 3, 3, dtype=torch.float64)
    rows = 4 * torch.arange(C)
    for k in range(3):
        for a in range(3):
            for b in range(3):
                for i in range(2):
                    for j in range(2):
                        dw4[k, :, a, b] += R[rows + 2 * i + j, (k * 4 + i + 2 - a) * 4 + j + 2 - b]
    # the windows (p, q) in {1, 2} x {1, 2} tile the HR image: their pixel sums add up to the sum of g
    db4 = torch.stack([sum(T48[(k * 4 + p) * 4 + q] for p in (1, 2) for q in (1, 2)) for k in range(3)])
    return dw2, db2, dw4, db4


def test_gather_is_the_window_image():
    """[2, 6, 10, 3] -> [2, 3, 5, 64]: pure data movement, so exact - the 48 window channels with their out-of-image zeros on all four
    sides (every pixel of a 3 x 5 image but the middle row's inner ones touches a border) and the zero channels 48..63."""
    from pesr_amd import ops
    N, H, W = 2, 3, 5
    g = _rand(torch.Generator().manual_seed(1), N, 2 * H, 2 * W, 3)
    gp = F.pad(g.permute(0, 3, 1, 2), (1, 1, 1, 1))                  # [N, 3, 2H+2, 2W+2]: index 2y-1+p of g is 2y+p here
    want = torch.zeros(N, H, W, 64)
    for k in range(3):
        for p in range(4):
            for q in range(4):
                want[..., (k * 4 + p) * 4 + q] = gp[:, k, p:p + 2 * H:2, q:q + 2 * W:2]
    got = ops.upsample_tail_gather(g.cuda()).cpu()
    assert got.shape == want.shape and torch.equal(got, want)
    assert (want[..., :48] == 0).any() and (want[..., :48] != 0).any()


def test_compose_and_chain_vs_float64():
    """C = 16, random W2, b2, W4, S, T (rows 48..63 of S and T random too: they must not count).  The kernels sum in double and round
    once, so helpers.close holds at its default 1e-6 of the tensor's maximum; accumulate = True adds to what the outputs held."""
    from pesr_amd import ops
    C = 16
    gen = torch.Generator().manual_seed(2)
    w2, b2, w4 = _rand(gen, 4 * C, C, 3, 3, scale=0.1), _rand(gen, 4 * C), _rand(gen, 3, C, 3, 3, scale=0.1)
    S, T = _rand(gen, 64, C, 3, 3), _rand(gen, 64)
    dev = [t.cuda() for t in (w2, b2, w4, S, T)]
    weff = ops.upsample_tail_compose(dev[0], dev[2]).cpu()
    assert weff.shape == (64, C, 3, 3) and not weff[48:].any()
    close(weff[:48], torch.einsum("mz,mcef->zcef", _A(w4), w2.double()), what="Weff")
    ref = _chain_ref(w2, b2, w4, S, T)
    names = ("dW2", "db2", "dW4", "db4")
    got = ops.upsample_tail_chain(*dev)
    for n, a, b in zip(names, got, ref):
        close(a, b, what=n)
    # accumulate: into given tensors, and only the wanted ones
    base = [_rand(gen, *r.shape) for r in ref]
    outs = tuple(t.cuda() for t in base)
    res = ops.upsample_tail_chain(*dev, outs=outs, accumulate=True)
    for n, o, r, b0, want in zip(names, outs, res, base, ref):
        assert r is o
        close(o, b0.double() + want, what=n + " accumulate")
    part = ops.upsample_tail_chain(*dev, want=(False, True, True, False))
    assert part[0] is None and part[3] is None
    assert torch.equal(part[1], got[1]) and torch.equal(part[2], got[2])
    # no bias on the first conv: the b2 T term is gone
    nob = ops.upsample_tail_chain(dev[0], None, *dev[2:])
    close(nob[2], _chain_ref(w2, torch.zeros(4 * C), w4, S, T)[2], what="dW4 without b2")


def _pair(C, seed):
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import Conv
    torch.manual_seed(seed)
    conv2, conv4 = Conv(C, 4 * C, 3), Conv(C, 3, 3)
    conv2.packed = PF.PackedConvWeights(ps=True)
    return conv2.cuda(), conv4.cuda()


@pytest.mark.parametrize("N,C,H,W", [(2, 64, 6, 8), (3, 16, 4, 4)])
def test_pair_collapsed_vs_unfused_vs_float64(monkeypatch, N, C, H, W):
    """The tail pair with the switch on and off, from the same weights, input and incoming gradient.  [2, 6, 8, 64]: not square, every
    border, more than one image; [3, 4, 4, 16]: the smallest shape at which every pixel is a border pixel.  The forwards are the same
    launches: equal bit for bit.  Against float64 torch autograd of conv -> pixel_shuffle -> conv on the CPU, the collapsed path's
    error (of the tensor's maximum) may be at most 3 x the un-fused HIP path's own error on the same inputs - the factor
    helpers.grads_vs_fp64 allows two fp32 evaluations of one quantity - with a floor of 1e-6."""
    from pesr_amd import functional as PF
    from pesr_amd import ops
    conv2, conv4 = _pair(C, 7)
    gen = torch.Generator().manual_seed(8)
    h0, gy = _rand(gen, N, H, W, C), _rand(gen, N, 2 * H, 2 * W, 3)
    params = (conv2.weight, conv2.bias, conv4.weight, conv4.bias)

    def run(on):
        monkeypatch.setattr(ops, "UPSAMPLE_TAIL", "1" if on else "0")
        h = h0.cuda().requires_grad_(True)
        y = PF.upsample_tail(h, conv2, conv4)
        assert (type(y.grad_fn).__name__ == "UpsampleTailFnBackward") is on
        grads = torch.autograd.grad(y, (h, *params), gy.cuda())
        return y.detach().cpu(), [t.cpu() for t in grads]

    y_on, g_on = run(True)
    y_off, g_off = run(False)
    assert torch.equal(y_on, y_off)

    h64 = h0.double().permute(0, 3, 1, 2).requires_grad_(True)
    p64 = [p.detach().cpu().double().requires_grad_(True) for p in params]
    y64 = F.conv2d(F.pixel_shuffle(F.conv2d(h64, p64[0], p64[1], padding=1), 2), p64[2], p64[3], padding=1)
    g64 = torch.autograd.grad(y64, (h64, *p64), gy.double().permute(0, 3, 1, 2))
    g64 = [g64[0].permute(0, 2, 3, 1)] + list(g64[1:])
    for name, a, b, r in zip(("dh", "dW2", "db2", "dW4", "db4"), g_on, g_off, g64):
        mx = r.abs().max().item()
        e_on, e_off = (a.double() - r).abs().max().item() / mx, (b.double() - r).abs().max().item() / mx
        print(f"[{N}x{H}x{W}x{C}] {name}: collapsed {e_on:.3e}, un-fused {e_off:.3e} of the maximum")
        assert e_on <= max(3.0 * e_off, 1e-6), f"{name}: collapsed {e_on:.3e} > 3 x the un-fused path's {e_off:.3e}"


def _pretrainer(C, depth, lr=5e-5):
    from model import Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1})
    G.load_state_dict(gen_sd(C, depth))
    G.cuda()
    return Trainer(G, optim_G=FlatAdam([p for p in G.parameters() if p.requires_grad], lr=lr, betas=(0.9, 0.999))), G


def test_toy_pretrain_step_switch_on_vs_off_and_captured(monkeypatch):
    """Generator with 64 channels, depth 2, batch 2, patch 8.  One pretrain step with the switch on and one with it off, from the same
    weights: the forward is untouched, so the losses are equal bit for bit; the parameters after the step within helpers.adam_close.
    Then the collapsed path under Trainer.capture_pretrain_step: replays equal eager steps bit for bit."""
    from pesr_amd import ops
    lr_rate = 5e-5
    data = [(detrand.image_batch((2, 3, 8, 8), 70 + i).cuda(), detrand.image_batch((2, 3, 32, 32), 80 + i).cuda()) for i in range(4)]
    monkeypatch.setattr(ops, "UPSAMPLE_TAIL", "0")
    tr_off, G_off = _pretrainer(64, 2, lr_rate)
    l_off = tr_off.pretrain_step(*data[0])["l1"].item()
    monkeypatch.setattr(ops, "UPSAMPLE_TAIL", "1")
    tr_on, G_on = _pretrainer(64, 2, lr_rate)
    l_on = tr_on.pretrain_step(*data[0])["l1"].item()
    assert l_on == l_off, (l_on, l_off)
    for (name, a), b in zip(G_on.named_parameters(), G_off.parameters()):
        adam_close(a, b, lr_rate, 1, name)

    tr_g, G_g = _pretrainer(64, 2, lr_rate)
    assert tr_g.pretrain_step(*data[0])["l1"].item() == l_on
    for t in (tr_on, tr_g):
        t.pretrain_step(*data[1])
    step = tr_g.capture_pretrain_step(*data[0])
    for lr, hr in data[2:]:
        assert tr_on.pretrain_step(lr, hr)["l1"].item() == step(lr, hr)["l1"].item()
    for a, b in zip(G_on.parameters(), G_g.parameters()):
        assert torch.equal(a, b)


def test_unset_switch_takes_the_path_only_where_it_gains(monkeypatch):
    """PESR_UPSAMPLE_TAIL unset: the collapsed backward from N H W C^2 = ops.TAIL_MIN_WORK up (its compose and chain launches do not
    shrink with the image; below that nothing is gained); "1" wherever it applies, "0" nowhere; never outside fp32 or for C % 16 != 0."""
    from pesr_amd import ops
    big, small, odd = (torch.empty(s, device="cuda") for s in ((16, 16, 16, 64), (4, 16, 16, 16), (16, 32, 32, 24)))
    assert big.shape[0] * big.shape[1] * big.shape[2] * 64 * 64 == ops.TAIL_MIN_WORK
    for mode, want in (("auto", (True, False)), ("1", (True, True)), ("0", (False, False))):
        monkeypatch.setattr(ops, "UPSAMPLE_TAIL", mode)
        assert (ops.upsample_tail_eligible(big, 64), ops.upsample_tail_eligible(small, 16)) == want, mode
        assert not ops.upsample_tail_eligible(odd, 24)
        with ops.use_precision("bf16"):
            assert not ops.upsample_tail_eligible(big, 64)
