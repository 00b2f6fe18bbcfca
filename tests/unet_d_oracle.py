"""float64 restatements for the U-Net discriminator's tests (docs/modes.md section 4v): torch on the CPU.  up2 is F.interpolate itself,
the GAN losses are the definitions of csrc/loss.hip (reference train.py:210-213, 244-253 and model/focal_loss.py with the torch-0.4
gradient through the focal weight AND the BCE term), the network is built from the module's own state_dict."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import model as OM

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(x64):
    """one fp32 ulp at |x| (float64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(x64.numpy()).astype(np.float32)).astype(np.float64))


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


# ---- bilinear x2 on NHWC maps ---------------------------------------------------------------------------------------------------------
def up2(x_nhwc64):
    return F.interpolate(x_nhwc64.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


def up2_t(g_nhwc64):
    """the adjoint of up2, by autograd of F.interpolate"""
    N, H2, W2, C = g_nhwc64.shape
    x = torch.zeros((N, H2 // 2, W2 // 2, C), dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(up2(x), x, g_nhwc64)
    return gx


# ---- the GAN losses on n logits ---------------------------------------------------------------------------------------------------------
def _term(x, t, focal, gam):
    """-> (value, d value / dx) per element; t a float"""
    p = torch.sigmoid(x)
    bce = F.binary_cross_entropy_with_logits(x, torch.full_like(x, t), reduction="none")
    if not focal:
        return bce, p - t
    pt = p * t + (1 - p) * (1 - t)
    w = (1 - pt).pow(gam)
    dw = torch.zeros_like(p) if gam == 0 else -gam * (1 - pt).pow(gam - 1) * (2 * t - 1) * p * (1 - p)
    return w * bce, dw * bce + w * (p - t)


def gan_loss(r, f, gan_type, side, focal=False, gam=1.0, scale=1.0):
    """r, f: float64 logits of one shape -> (scale * mean loss, scale * dloss/dr, scale * dloss/df)"""
    n = r.numel()
    fo = focal and side == 1
    zero = torch.zeros_like(r)
    if gan_type == "SGAN":
        if side == 0:
            v1, g1 = _term(r, 1.0, False, 0.0)
            v2, g2 = _term(f, 0.0, False, 0.0)
            val, gr, gf = v1 + v2, g1, g2
        else:
            val, gf = _term(f, 1.0, fo, gam)
            gr = zero
    elif gan_type == "RSGAN":
        if side == 0:
            val, g = _term(r - f, 1.0, False, 0.0)
            gr, gf = g, -g
        else:
            val, g = _term(f - r, 1.0, fo, gam)
            gf, gr = g, -g
    else:
        mr, mf = r.mean(), f.mean()
        va, ga = _term(r - mf, 1.0 if side == 0 else 0.0, fo, gam)
        vb, gb = _term(f - mr, 0.0 if side == 0 else 1.0, fo, gam)
        val = 0.5 * (va + vb)
        gr = 0.5 * (ga - gb.sum() / n)
        gf = 0.5 * (gb - ga.sum() / n)
    return scale * val.sum() / n, scale * gr / n, scale * gf / n


class _Focal(torch.autograd.Function):
    """mean focal loss with the closed-form gradient above, for float64 autograd through a network"""

    @staticmethod
    def forward(ctx, x, t, gam):
        val, dx = _term(x, t, True, gam)
        ctx.save_for_backward(dx)
        return val.mean()

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return g * dx / dx.numel(), None, None


def gan_loss_autograd(r, f, gan_type, side, focal=False, gam=1.0, scale=1.0):
    """the same loss as a differentiable float64 scalar of the logit tensors r, f"""
    def L(x, t):
        if focal and side == 1:
            return _Focal.apply(x, t, gam)
        return F.binary_cross_entropy_with_logits(x, torch.full_like(x, t))
    if gan_type == "SGAN":
        out = L(r, 1.0) + L(f, 0.0) if side == 0 else L(f, 1.0)
    elif gan_type == "RSGAN":
        out = L(r - f, 1.0) if side == 0 else L(f - r, 1.0)
    else:
        a, b = (1.0, 0.0) if side == 0 else (0.0, 1.0)
        out = 0.5 * (L(r - f.mean(), a) + L(f - r.mean(), b))
    return scale * out


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def unet_d(sd, x, slope=0.2, kinks=None):
    """sd: the module's state_dict as float64 tensors (the weights leaves of autograd; under spectral norm weight_orig / weight_u /
    weight_v, and u, v are updated in place as a training forward does); x [B, 3, H, W] float64 -> [B, 1, H, W].  kinks: a list that
    receives, per LeakyReLU, the smallest |pre-activation| over the layer's largest - how close the input comes to a kink, where
    the gradient jumps and an fp32 evaluation may land on the other side."""
    def conv(i, h, stride=1):
        if f"conv{i}.weight_orig" in sd:
            w = OM.spectral_normalize(sd[f"conv{i}.weight_orig"], sd[f"conv{i}.weight_u"], sd[f"conv{i}.weight_v"], True)
        else:
            w = sd[f"conv{i}.weight"]
        z = F.conv2d(h, w, sd.get(f"conv{i}.bias"), stride=stride, padding=1)
        if kinks is not None and i < 9:
            kinks.append(float(z.detach().abs().min() / z.detach().abs().max()))
        return z

    act = lambda h: F.leaky_relu(h, slope)
    up = lambda h: F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=False)
    x0 = act(conv(0, x))
    x1 = act(conv(1, x0, 2))
    x2 = act(conv(2, x1, 2))
    x3 = act(conv(3, x2, 2))
    x4 = act(conv(4, up(x3))) + x2
    x5 = act(conv(5, up(x4))) + x1
    x6 = act(conv(6, up(x5))) + x0
    return conv(9, act(conv(8, act(conv(7, x6)))))


def leaves(module):
    """the module's state_dict as float64 CPU tensors; the parameters require grad"""
    params = {k for k, _ in module.named_parameters()}
    return {k: v.detach().cpu().double().clone().requires_grad_(k in params) for k, v in module.state_dict().items()}
