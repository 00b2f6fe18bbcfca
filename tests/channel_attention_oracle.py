"""The channel attention of docs/modes.md section 4u restated in float64 (torch on the CPU): the definition itself - the reference has
no such block - with every intermediate, the closed-form backward, the error bound of an fp32 sum in any order, float64 restatements
of ResBlock / Generator built from a state_dict, and the makers of the tests' inputs.

    m[n,c] = (1/HW) sum_p t[n,p,c]       h[n,j] = relu(sum_c W1[j,c] m[n,c] + B1[j])       s[n,c] = sigmoid(sum_j W2[c,j] h[n,j] + B2[c])
    y = x + a t s[n,c]
    gx = gy     ds[n,c] = a sum_p gy t     dz2 = ds s (1 - s)     dh = dz2 W2     dz1 = dh [h > 0]     dm = dz1 W1
    dW2 = dz2^T h   dB2 = sum_n dz2   dW1 = dz1^T m   dB1 = sum_n dz1       gt = a gy s + dm / HW
"""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                                                    # the unit roundoff of float32


def _t(x):
    if torch.is_tensor(x):
        return x.detach().cpu().double()
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def pool(t):
    """[N, H, W, C] -> m [N, C]"""
    t = _t(t)
    return t.reshape(t.shape[0], -1, t.shape[-1]).mean(1)


def ds_sum(gy, t, a):
    gy, t = _t(gy), _t(t)
    return a * (gy * t).reshape(t.shape[0], -1, t.shape[-1]).sum(1)


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def sum_bound(terms, scale, result):
    """The issue's bound on an fp32 sum of n = HW terms per (image, channel) in ANY order, scaled by `scale` and rounded once more:
    gamma(n) * scale * sum |terms|  +  one ulp of the (float32) result.  terms: [N, H, W, C] float64."""
    terms = _t(terms)
    n = terms.shape[1] * terms.shape[2]
    mag = terms.abs().reshape(terms.shape[0], -1, terms.shape[-1]).sum(1)
    ulp = np.spacing(np.abs(_t(result).numpy().astype(np.float32))).astype(np.float64)
    return gamma(n) * abs(scale) * mag + torch.as_tensor(ulp)


def gate(m, w1, b1, w2, b2):
    """-> dict(z1, h, z2, s);  w1 [R, C(,1,1)], w2 [C, R(,1,1)]"""
    m, b1, b2 = _t(m), _t(b1), _t(b2)
    w1 = _t(w1).reshape(b1.shape[0], -1)
    w2 = _t(w2).reshape(b2.shape[0], -1)
    z1 = m @ w1.T + b1
    h = z1.clamp(min=0)
    z2 = h @ w2.T + b2
    return dict(z1=z1, h=h, z2=z2, s=torch.sigmoid(z2))


def gate_backward(ds, s, h, m, w1, w2):
    """The closed form, with the forward's s, h, m as arguments (the kernels' contract: the ReLU is open where the h given is > 0)
    -> dict(dm, dw1, db1, dw2, db2)"""
    ds, s, h, m = _t(ds), _t(s), _t(h), _t(m)
    w1 = _t(w1).reshape(h.shape[1], -1)
    w2 = _t(w2).reshape(s.shape[1], -1)
    dz2 = ds * s * (1.0 - s)
    dz1 = (dz2 @ w2) * (h > 0)
    return dict(dm=dz1 @ w1, dw1=dz1.T @ m, db1=dz1.sum(0), dw2=dz2.T @ h, db2=dz2.sum(0))


def node(x, t, w1, b1, w2, b2, a):
    """y = x + a t s, differentiable float64 torch (inputs may require grad): x, t [N, H, W, C]"""
    R, C = b1.shape[0], b2.shape[0]
    m = t.reshape(t.shape[0], -1, C).mean(1)
    h = torch.relu(m @ w1.reshape(R, C).T + b1)
    s = torch.sigmoid(h @ w2.reshape(C, R).T + b2)
    return x + a * t * s[:, None, None, :]


def node_grads(x, t, w1, b1, w2, b2, a, gy):
    """float64 autograd of node(): -> (y, [gx, gt, gw1, gb1, gw2, gb2]), shaped like the inputs"""
    leaves = [_t(v).clone().requires_grad_(True) for v in (x, t, w1, b1, w2, b2)]
    y = node(*leaves, a)
    y.backward(_t(gy))
    return y.detach(), [v.grad for v in leaves]


# ---- float64 restatements of the modules, from a state_dict (keys of pesr_amd.model: body.0.weight, body.2.weight, ca.squeeze.weight ...)
def resblock(sd, x, res_scale, prefix=""):
    """ResBlock(bias or not, no BN, ReLU) with or without channel attention, NCHW float64, differentiable in the tensors of sd"""
    g = lambda k: sd.get(prefix + k)
    r = F.relu(F.conv2d(x, g("body.0.weight"), g("body.0.bias"), padding=1))
    t = F.conv2d(r, g("body.2.weight"), g("body.2.bias"), padding=1)
    if g("ca.squeeze.weight") is None:
        return x + res_scale * t
    m = t.mean((2, 3), keepdim=True)
    h = F.relu(F.conv2d(m, g("ca.squeeze.weight"), g("ca.squeeze.bias")))
    s = torch.sigmoid(F.conv2d(h, g("ca.excite.weight"), g("ca.excite.bias")))
    return x + res_scale * t * s


def generator(sd, x, depth, res_scale):
    """The x4 Generator, NCHW float64, differentiable in the tensors of sd"""
    c = lambda k, v, p: F.conv2d(v, sd[k + ".weight"], sd[k + ".bias"], padding=p)
    feat = c("embed", c("sub_mean", x, 0), 1)
    h = feat
    for i in range(depth):
        h = resblock(sd, h, res_scale, f"body.{i}.")
    h = c(f"body.{depth}", h, 1) + feat
    h = F.pixel_shuffle(c("upsample.0", h, 1), 2)
    h = F.pixel_shuffle(c("upsample.2", h, 1), 2)
    return c("add_mean", c("upsample.4", h, 1), 0)


def double_leaves(state_dict):
    """state_dict -> {key: float64 CPU leaf that requires grad}"""
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in state_dict.items()}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def features(shape, seed, scale=0.5, offset=0.1):
    """A seeded [N, H, W, C] float32 map on the scale of trunk activations, both signs, a per-channel offset so that the means differ"""
    g = np.random.default_rng(seed)
    t = g.standard_normal(shape) * scale + offset * g.standard_normal((1, 1, 1, shape[-1]))
    return t.astype(np.float32)


def gate_case(N, C, reduction, seed):
    """Seeded gate inputs with the hard rows built in: -> dict(m, w1, b1, w2, b2, ds) float32 numpy.  Image 0 has hidden unit 0 shut
    (pre-activation -1: h exactly 0), the last image (when there is another) has it open (+1); channels 0 and 1 have pre-activations
    of exactly +20 and -20 (a saturated sigmoid); the other rows are ordinary.  No pre-activation of a hidden unit lies within 1e-3
    of 0 (the draw is repeated with the next seed until that holds), so fp32 and float64 agree on which ReLUs are open."""
    R = C // reduction
    for attempt in range(100):
        g = np.random.default_rng(seed + 1000 * attempt)
        m = g.standard_normal((N, C)) * 0.3
        w1 = (g.standard_normal((R, C)) / np.sqrt(C)).astype(np.float32)
        b1 = (g.standard_normal(R) * 0.1).astype(np.float32)
        w2 = (g.standard_normal((C, R)) / np.sqrt(R)).astype(np.float32)
        b2 = (g.standard_normal(C) * 0.1).astype(np.float32)
        ds = g.standard_normal((N, C)).astype(np.float32)
        u = w1[0].astype(np.float64)
        for n, want in ((0, -1.0),) + (((N - 1, 1.0),) if N > 1 else ()):     # move m[n] along w1[0] until unit 0 sits at `want`
            m[n] += (want - (m[n] @ u + b1[0])) / (u @ u) * u
        m = m.astype(np.float32)
        b2[0], b2[1] = 20.0, -20.0
        w2[0, :], w2[1, :] = 0.0, 0.0
        z1 = m.astype(np.float64) @ w1.astype(np.float64).T + b1
        if np.abs(z1).min() > 1e-3:
            assert z1[0, 0] < -0.5 and (N == 1 or z1[N - 1, 0] > 0.5)
            return dict(m=m, w1=w1, b1=b1, w2=w2, b2=b2, ds=ds)
    raise AssertionError("gate_case: no draw with every hidden pre-activation away from 0")


def rel_err(got, want):
    """max |got - want| / max |want|, the project's per-tensor gradient measure"""
    got, want = _t(got).reshape(-1), _t(want).reshape(-1)
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))
