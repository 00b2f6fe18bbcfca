"""The contextual loss of docs/modes.md section 4r restated in float64 (torch on the CPU): every intermediate, the value, the closed-form
gradient with the selections a, b as arguments (default: its own), the first-order error bounds of the fp32 kernels
(pesr_amd/csrc/cx.hip), and the two makers of the tests' inputs.

    mu = mean_j y_j     xb = x - mu, yb = y - mu     xh = xb / sqrt(|xb|^2 + 1e-12), yh likewise      d_ij = (1 - xh_i . yh_j) / 2
    m_i = min_k d_ik = d_i,b(i)     w_ij = exp((1 - d_ij / (m_i + 1e-5)) / h)     S_i = sum_k w_ik     c_ij = w_ij / S_i
    CX = (1 / P) sum_j c_a(j),j  with a(j) = arg max_i c_ij     L = -log CX

With a, b fixed and q = -gL / (P CX), T_i = sum_{j: a(j) = i} c_ij, U_i = sum_k c_ik ([a(k) = i] - T_i) d_ik / (h (m_i + eps)^2):

    E_ik = dL/dd_ik = q (-c_ik ([a(k) = i] - T_i) / (h (m_i + eps)) + [k = b(i)] U_i)
    g_xh = -E yh / 2      dL/dx_i = (g_xh_i - xh_i (xh_i . g_xh_i)) / sqrt(|xb_i|^2 + 1e-12)
"""
import numpy as np
import torch

U32 = 2.0 ** -24                                                    # the unit roundoff of float32
EPS, TINY = 1e-5, 1e-12


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def points(f):
    """[N, H, W, C] -> float64 torch [N, P, C], row-major points"""
    f = _t(f)
    return f.reshape(f.shape[0], -1, f.shape[-1])


def normalize(fa, fb):
    """-> mu [N, 1, C], xb, yb, rx [N, P, 1] = 1 / sqrt(|xb|^2 + 1e-12), ry, xh, yh"""
    x, y = points(fa), points(fb)
    mu = y.mean(dim=1, keepdim=True)
    xb, yb = x - mu, y - mu
    rx = 1.0 / torch.sqrt((xb * xb).sum(-1, keepdim=True) + TINY)
    ry = 1.0 / torch.sqrt((yb * yb).sum(-1, keepdim=True) + TINY)
    return mu, xb, yb, rx, ry, xb * rx, yb * ry


def lowest_argmin(D, dim):
    """The lowest index among equal minima along dim"""
    m = D.min(dim=dim, keepdim=True).values
    n = D.shape[dim]
    idx = torch.arange(n).reshape([-1 if i == dim % D.dim() else 1 for i in range(D.dim())]).expand_as(D)
    return torch.where(D == m, idx, torch.full_like(idx, n)).min(dim=dim).values


def from_dist(D, h=0.5, a=None, b=None):
    """D float64 [N, P, P] -> dict(m, b, w, S, c, cmax, a, CX, L); a, b given: used instead of the arg max / arg min"""
    D = _t(D)
    b = lowest_argmin(D, 2) if b is None else torch.as_tensor(np.asarray(b)).long()
    m = D.gather(2, b.unsqueeze(2))                                   # [N, P, 1]
    w = torch.exp((1.0 - D / (m + EPS)) / h)
    S = w.sum(2, keepdim=True)
    c = w / S
    a = lowest_argmin(-c, 1) if a is None else torch.as_tensor(np.asarray(a)).long()
    cmax = c.gather(1, a.unsqueeze(1)).squeeze(1)                     # [N, P]
    CX = cmax.mean(1)
    return dict(D=D, m=m.squeeze(2), b=b, w=w, S=S.squeeze(2), c=c, cmax=cmax, a=a, CX=CX, L=-torch.log(CX))


def stages(fa, fb, h=0.5, a=None, b=None):
    """Everything, float64 torch tensors"""
    mu, xb, yb, rx, ry, xh, yh = normalize(fa, fb)
    out = from_dist((1.0 - xh @ yh.transpose(1, 2)) / 2.0, h, a, b)
    out.update(mu=mu.squeeze(1), xb=xb, yb=yb, inv=rx.squeeze(2), xh=xh, yh=yh)
    return out


def loss(fa, fb, h=0.5):
    """float64 numpy [N]"""
    return stages(fa, fb, h)["L"].numpy()


def e_matrix(D, m, b, S, a, cmax, CX, gL, h=0.5):
    """E = dL/dD [N, P, P] in float64 from these quantities (the oracle's own, or a device's) with a, b held fixed"""
    D, m, S, cmax, CX, gL = _t(D), _t(m).unsqueeze(2), _t(S).unsqueeze(2), _t(cmax), _t(CX), _t(gL)
    a, b = torch.as_tensor(np.asarray(a)).long(), torch.as_tensor(np.asarray(b)).long()
    N, P, _ = D.shape
    c = torch.exp((1.0 - D / (m + EPS)) / h) / S
    sel = torch.zeros_like(D)                                         # [a(k) = i]
    sel.scatter_(1, a.unsqueeze(1), 1.0)
    T = torch.zeros(N, P, dtype=torch.float64).scatter_add_(1, a, cmax).unsqueeze(2)
    G = c * (sel - T)
    U = (G * D).sum(2, keepdim=True) / (h * (m + EPS) ** 2)
    q = (-gL / (P * CX)).reshape(N, 1, 1)
    E = -G / (h * (m + EPS))
    E.scatter_add_(2, b.unsqueeze(2), U)
    return q * E


def grad(fa, fb, gL, h=0.5, a=None, b=None):
    """The closed form: -> dict(E, gxh, gf [N, H, W, C]) float64 numpy, plus the stages"""
    s = stages(fa, fb, h, a, b)
    E = e_matrix(s["D"], s["m"], s["b"], s["S"], s["a"], s["cmax"], s["CX"], gL, h)
    gxh = -0.5 * E @ s["yh"]
    gx = (gxh - s["xh"] * (s["xh"] * gxh).sum(-1, keepdim=True)) * s["inv"].unsqueeze(2)
    return dict(s, E=E, gxh=gxh, gf=gx.reshape(np.asarray(fa).shape).numpy())


# ---- first-order bounds of the fp32 kernels: one rounding per operation, in any order ----------------------------------------------------
def normalize_bound(fa, fb):
    """|xh - xh64| and |yh - yh64| per element.  mu is a double sum rounded once (u |mu|), xb = fl(x - mu) (u |xb| more), the squared
    length is summed in double from those xb (so r inherits r^2 sum |xb| |dxb| relatively, plus its own rounding), xh = fl(xb r).
    The rounding of mu alone reaches its u |mu| in some channel of every image, so the first-order sum is nearly attained where
    |xb| << |mu|; the factor 1 + 8 u stands for the products of the first-order terms that the sum leaves out."""
    mu, xb, yb, rx, ry, xh, yh = normalize(fa, fb)
    out = []
    for vb, r, vh in ((xb, rx, xh), (yb, ry, yh)):
        dvb = U32 * (mu.abs() + vb.abs())
        rel_r = U32 + r * r * (vb.abs() * dvb).sum(-1, keepdim=True)
        out.append(((1 + 8 * U32) * (r * dvb + vh.abs() * (rel_r + U32))).numpy())
    return out


def dist_bound(xh, yh):
    """|D - D64| per entry for D64 from the same xh, yh: C products and C additions, then d = fma(-0.5, s, 0.5), one rounding"""
    xh, yh = _t(xh), _t(yh)
    C = xh.shape[-1]
    s = xh.abs() @ yh.abs().transpose(1, 2)
    d = (1.0 - xh @ yh.transpose(1, 2)) / 2.0
    return ((C + 8) * U32 * 0.5 * s + U32 * d.abs()).numpy()


def gxh_bound(E, yh):
    """|g_xh - g_xh64| per element for g_xh64 = -E yh / 2 from the same E, yh: P products and P additions (the half is exact)"""
    E, yh = _t(E), _t(yh)
    return ((E.shape[-1] + 8) * U32 * 0.5 * (E.abs() @ yh.abs())).numpy()


# ---- the tests' inputs --------------------------------------------------------------------------------------------------------------------
def features(seed, n, h, w, c, regime):
    """(fa, fb) float32 [n, h, w, c]: non-negative, channel magnitudes spread over e^-1 .. e^1 as behind a ReLU;
    matched: fa = relu(fb + 0.5 noise) - every sr point has its own hr point nearest; unmatched: fa = relu(fb + 2 noise)."""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(-1.0, 1.0, size=c))
    fb = np.maximum(rng.standard_normal((n, h, w, c)) * scale + 0.3 * scale, 0.0)
    noise = rng.standard_normal((n, h, w, c)) * scale
    fa = np.maximum(fb + {"matched": 0.5, "unmatched": 2.0}[regime] * noise, 0.0)
    return fa.astype(np.float32), fb.astype(np.float32)
