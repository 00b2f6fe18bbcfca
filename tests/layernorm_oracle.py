"""The channel LayerNorm of docs/modes.md section 4x restated in plain torch on the CPU: the definition, autograd for the gradients, the
same function in float64 (the oracle) and in float32 (whose distance from the oracle is the *fp32 reference error* the kernels'
tolerance is a multiple of), the closed-form backward, and float64 restatements of the WindowAttention module and of a Generator
whose blocks carry the norm.

    x [P, C], per pixel p:   mean = (1/C) sum_c x      var = (1/C) sum_c (x - mean)^2      rstd = 1 / sqrt(var + eps)
                             xh = (x - mean) rstd      y = xh gamma + beta                  eps = 1e-5
    backward:                g = dy gamma              dx = rstd (g - mean_c(g) - xh mean_c(g xh))
                             dgamma_c = sum_p dy xh    dbeta_c = sum_p dy
"""
import numpy as np
import torch
import torch.nn.functional as F

import window_attention_oracle as WO

EPS = 1e-5
U32 = WO.U32
rel_err = WO.rel_err
tolerance = WO.tolerance          # 4 x the fp32 reference error of the same case, with a floor of 8 * 2^-24
normal_like = WO.normal_like


def layernorm(x, gamma, beta, eps=EPS):
    """x [..., C] -> y, in x's dtype, differentiable; the centred two-pass variance"""
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d * (1.0 / torch.sqrt(var + eps)) * gamma + beta


def one_pass_layernorm(x, gamma, beta, eps=EPS):
    """The form the kernels must NOT be: var = E[x^2] - mean^2, which cancels where the mean is large (tests only: it has to miss
    the tolerance on the large-mean cases, or these would not catch it)"""
    mean = x.mean(dim=-1, keepdim=True)
    var = (x * x).mean(dim=-1, keepdim=True) - mean * mean
    return (x - mean) * (1.0 / torch.sqrt(var.clamp_min(0) + eps)) * gamma + beta


def grads(x, gamma, beta, dy, dtype=torch.float64, fn=layernorm):
    """-> (y, dx, dgamma, dbeta) by autograd, computed in dtype and returned as float64"""
    t = [torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_(True) for a in (x, gamma, beta)]
    y = fn(*t)
    y.backward(torch.as_tensor(np.asarray(dy)).to(dtype))
    return (y.detach().double(),) + tuple(a.grad.double() for a in t)


def analytic_backward(x, gamma, dy, eps=EPS):
    """The closed form of the module docstring in float64 -> (dx, dgamma, dbeta)"""
    x, gamma, dy = (torch.as_tensor(np.asarray(a)).double() for a in (x, gamma, dy))
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dx, flat(dy * xh).sum(0), flat(dy).sum(0)


# ---- the kernel cases ------------------------------------------------------------------------------------------------------------------
NAMES = ("y", "dx", "dgamma", "dbeta")
_CASES = {}


def inputs(P, C, kind="normal"):
    """Seeded float32 numpy: x [P, C] (normal: unit normals; big-mean: 1000 + n; features: 13 + 40 n, the trunk's features in front of a
    block; zero-rows: unit normals with every third row zero), gamma = 1 + 0.5 n, beta and dy unit normals"""
    seed = 3000 + 31 * P + C
    x = normal_like((P, C), seed)
    if kind == "big-mean":
        x = (np.float32(1000.0) + x).astype(np.float32)
    elif kind == "features":
        x = (np.float32(13.0) + np.float32(40.0) * x).astype(np.float32)
    elif kind == "zero-rows":
        x[::3] = 0.0
    else:
        assert kind == "normal", kind
    gamma = (np.float32(1.0) + np.float32(0.5) * normal_like((C,), seed + 1)).astype(np.float32)
    return x, gamma, normal_like((C,), seed + 2), normal_like((P, C), seed + 3)


def case(P, C, kind="normal"):
    """The shared, unchanging reference of a kernel case: dict(x, gamma, beta, dy float32 numpy; want: {name: float64}; ref: {name: the
    fp32 reference error - the same function in float32 on the CPU against float64, max error over the float64 maximum})"""
    key = (P, C, kind)
    if key not in _CASES:
        x, gamma, beta, dy = inputs(P, C, kind)
        want = dict(zip(NAMES, grads(x, gamma, beta, dy, torch.float64)))
        got32 = dict(zip(NAMES, grads(x, gamma, beta, dy, torch.float32)))
        _CASES[key] = dict(x=x, gamma=gamma, beta=beta, dy=dy, want=want, ref={n: rel_err(got32[n], want[n]) for n in NAMES})
    return _CASES[key]


# ---- float64 restatements of the modules, from a state_dict ----------------------------------------------------------------------------
def _pre(sd, x, prefix):
    """LN(x) where the block has a norm, x where it has none; NCHW"""
    if prefix + "norm.weight" not in sd:
        return x
    return layernorm(x.permute(0, 2, 3, 1), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"]).permute(0, 3, 1, 2)


def qkv_of(sd, x, prefix=""):
    return F.conv2d(_pre(sd, x, prefix), sd[prefix + "qkv.weight"], sd[prefix + "qkv.bias"], padding=1)


def block(sd, x, shift, prefix=""):
    """WindowAttention with norm="ln": x + proj(attention(qkv(LN(x)))), the skip from the un-normalised x; NCHW, differentiable in the
    tensors of sd"""
    o = WO.attention(qkv_of(sd, x, prefix).permute(0, 2, 3, 1), shift).permute(0, 3, 1, 2)
    return x + F.conv2d(o, sd[prefix + "proj.weight"], sd[prefix + "proj.bias"], padding=1)


def generator(sd, x, depth, res_scale, taps=None):
    """The x4 Generator with the window-attention blocks its state_dict has, each with the norm it has (and channel attention where the
    state_dict has that), NCHW.  taps: a dict that receives the features in front of each block ("in.<i>") and its qkv ("qkv.<i>")."""
    c = lambda k, v, p: F.conv2d(v, sd[k + ".weight"], sd[k + ".bias"], padding=p)
    feat = c("embed", c("sub_mean", x, 0), 1)
    h, j = feat, 0
    for i in range(depth):
        h = WO.CO.resblock(sd, h, res_scale, f"body.{i}.")
        if f"wattn.{i}.qkv.weight" in sd:
            if taps is not None:
                taps[f"in.{i}"] = h.detach()
                taps[f"qkv.{i}"] = qkv_of(sd, h, f"wattn.{i}.").detach()
            h = block(sd, h, 4 * (j % 2), f"wattn.{i}.")
            j += 1
    h = c(f"body.{depth}", h, 1) + feat
    h = F.pixel_shuffle(c("upsample.0", h, 1), 2)
    h = F.pixel_shuffle(c("upsample.2", h, 1), 2)
    return c("add_mean", c("upsample.4", h, 1), 0)


def largest_logit(qkv_nchw, shift):
    """The largest |logit| of window attention over a qkv map [1, 3 D, H, W]"""
    parts = []
    WO.attention(qkv_nchw.permute(0, 2, 3, 1), shift, parts)
    return max(float(S.abs().max()) for _, _, S in parts)
