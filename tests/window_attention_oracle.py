"""The window self-attention of docs/modes.md section 4w restated in plain torch on the CPU: an explicit loop over the windows with explicit
masks, autograd for the gradients, the same function in float64 (the oracle) and in float32 (whose distance from the oracle is the
*fp32 reference error* the kernel's tolerance is a multiple of), the closed-form backward, and float64 restatements of the
WindowAttention module and of a Generator with such blocks.

    window w = 8, head width d = 32, tau = 1 / sqrt(32); the window grid has its origin at (-s, -s): window (a, b) covers rows
    8a - s .. 8a - s + 7 and the same in x; positions outside the image are no tokens.
    per window and head over its tokens:   S = tau q k^T    A = softmax_rows(S)    o = A v
    dv = A^T do    dA = do v^T    dS = A * (dA - rowsum(dA * A))    dq = tau dS k    dk = tau dS^T q
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import channel_attention_oracle as CO
from oracle import detrand

WINDOW, HEAD = 8, 32
TAU = 1.0 / math.sqrt(HEAD)
U32 = 2.0 ** -24


def windows(H, W, shift):
    """-> [(rows, cols)]: for every window of the grid the image rows and columns inside it (lists of indices, never empty)"""
    out = []
    for a in range(-(-(H + shift) // WINDOW)):
        rows = [y for y in range(WINDOW * a - shift, WINDOW * a - shift + WINDOW) if 0 <= y < H]
        for b in range(-(-(W + shift) // WINDOW)):
            cols = [x for x in range(WINDOW * b - shift, WINDOW * b - shift + WINDOW) if 0 <= x < W]
            out.append((rows, cols))
    return out


def query_counts(H, W, shift):
    """How often each pixel is a query: the windows partition the image exactly where this is 1 everywhere."""
    n = torch.zeros(H, W, dtype=torch.int64)
    for rows, cols in windows(H, W, shift):
        assert rows and cols
        n[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] += 1
    return n


def attention(qkv, shift, parts=None):
    """qkv [N, H, W, 3 D] (q | k | v, heads of 32 channels) -> out [N, H, W, D], in qkv's dtype, differentiable.  parts: a list that
    receives (window index, head, S) for every window and head of image 0 (the logits, for the saturation test)."""
    N, H, W, D3 = qkv.shape
    D = D3 // 3
    assert D3 == 3 * D and D % HEAD == 0
    pieces = []
    for wi, (rows, cols) in enumerate(windows(H, W, shift)):
        r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
        tok = qkv[:, r0:r1, c0:c1, :].reshape(N, -1, D3)                  # the window's valid tokens, row-major
        o = []
        for h in range(D // HEAD):
            q, k, v = (tok[:, :, j * D + h * HEAD: j * D + (h + 1) * HEAD] for j in range(3))
            S = TAU * (q @ k.transpose(1, 2))
            if parts is not None:
                parts.append((wi, h, S[0].detach()))
            S = S - S.max(dim=2, keepdim=True).values.detach()
            P = torch.exp(S)
            A = P / P.sum(dim=2, keepdim=True)
            o.append(A @ v)
        pieces.append((r0, r1, c0, c1, torch.cat(o, dim=2).reshape(N, r1 - r0, c1 - c0, D)))
    # the windows partition the image: a row of windows side by side, the rows below one another (no in-place writes under autograd)
    grid_h, grid_w = -(-(H + shift) // WINDOW), -(-(W + shift) // WINDOW)
    return torch.cat([torch.cat([pieces[a * grid_w + b][4] for b in range(grid_w)], dim=2) for a in range(grid_h)], dim=1)


def attention_grads(qkv, dout, shift, dtype=torch.float64):
    """-> (out, dqkv) by autograd, both computed in dtype and returned as float64"""
    x = torch.as_tensor(np.asarray(qkv)).to(dtype).clone().requires_grad_(True)
    out = attention(x, shift)
    out.backward(torch.as_tensor(np.asarray(dout)).to(dtype))
    return out.detach().double(), x.grad.double()


def analytic_backward(qkv, dout, shift):
    """The closed form of the module docstring in float64 -> dqkv"""
    qkv, dout = torch.as_tensor(np.asarray(qkv)).double(), torch.as_tensor(np.asarray(dout)).double()
    N, H, W, D3 = qkv.shape
    D = D3 // 3
    dqkv = torch.zeros_like(qkv)
    for rows, cols in windows(H, W, shift):
        r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
        tok = qkv[:, r0:r1, c0:c1, :].reshape(N, -1, D3)
        g = dout[:, r0:r1, c0:c1, :].reshape(N, -1, D)
        d = torch.zeros_like(tok)
        for h in range(D // HEAD):
            sl = [slice(j * D + h * HEAD, j * D + (h + 1) * HEAD) for j in range(3)]
            q, k, v = (tok[:, :, s] for s in sl)
            do = g[:, :, h * HEAD:(h + 1) * HEAD]
            A = torch.softmax(TAU * (q @ k.transpose(1, 2)), dim=2)
            dA = do @ v.transpose(1, 2)
            dS = A * (dA - (dA * A).sum(2, keepdim=True))
            d[:, :, sl[0]] = TAU * (dS @ k)
            d[:, :, sl[1]] = TAU * (dS.transpose(1, 2) @ q)
            d[:, :, sl[2]] = A.transpose(1, 2) @ do
        dqkv[:, r0:r1, c0:c1, :] = d.reshape(N, r1 - r0, c1 - c0, D3)
    return dqkv


def rel_err(got, want):
    return CO.rel_err(got, want)


def normal_like(shape, seed):
    """Seeded float32 numpy of unit variance and zero mean, bell-shaped: the sum of three of oracle.detrand's uniforms on [-1, 1]"""
    return sum(detrand.uniform(shape, seed * 3 + i) for i in range(3)).numpy().astype(np.float32)


_CASES = {}


def case(N, H, W, D, shift, qk_scale=1.0):
    """The shared, unchanging reference of a kernel case: dict(qkv, dout float32 numpy; out, dqkv float64; ref_out, ref_dqkv: the fp32
    reference errors (the same function in float32 on the CPU against float64, max error over the float64 maximum))"""
    key = (N, H, W, D, shift, qk_scale)
    if key not in _CASES:
        seed = 1000 + 7 * N + 13 * H + 17 * W + D + shift
        qkv = normal_like((N, H, W, 3 * D), seed)
        qkv[..., :2 * D] *= np.float32(qk_scale)
        dout = normal_like((N, H, W, D), seed + 1)
        out, dqkv = attention_grads(qkv, dout, shift, torch.float64)
        out32, dqkv32 = attention_grads(qkv, dout, shift, torch.float32)
        _CASES[key] = dict(qkv=qkv, dout=dout, out=out, dqkv=dqkv, ref_out=rel_err(out32, out), ref_dqkv=rel_err(dqkv32, dqkv))
    return _CASES[key]


def tolerance(ref_err):
    """4 x the fp32 reference error of the same case (two independent fp32 orderings, x 2; a device expf that need not be the host's,
    x 2 again), with a floor of 8 * 2^-24"""
    return max(4.0 * ref_err, 8.0 * U32)


# ---- float64 restatements of the modules, from a state_dict ------------------------------------------------------------------------------
def block(sd, x, shift, prefix=""):
    """WindowAttention, NCHW float64, differentiable in the tensors of sd"""
    u = F.conv2d(x, sd[prefix + "qkv.weight"], sd[prefix + "qkv.bias"], padding=1)
    o = attention(u.permute(0, 2, 3, 1), shift).permute(0, 3, 1, 2)
    return x + F.conv2d(o, sd[prefix + "proj.weight"], sd[prefix + "proj.bias"], padding=1)


def generator(sd, x, depth, res_scale):
    """The x4 Generator with the window-attention blocks its state_dict has (and channel attention where it has that), NCHW float64"""
    c = lambda k, v, p: F.conv2d(v, sd[k + ".weight"], sd[k + ".bias"], padding=p)
    feat = c("embed", c("sub_mean", x, 0), 1)
    h, j = feat, 0
    for i in range(depth):
        h = CO.resblock(sd, h, res_scale, f"body.{i}.")
        if f"wattn.{i}.qkv.weight" in sd:
            h = block(sd, h, 4 * (j % 2), f"wattn.{i}.")
            j += 1
    h = c(f"body.{depth}", h, 1) + feat
    h = F.pixel_shuffle(c("upsample.0", h, 1), 2)
    h = F.pixel_shuffle(c("upsample.2", h, 1), 2)
    return c("add_mean", c("upsample.4", h, 1), 0)
