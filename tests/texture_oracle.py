"""The texture loss of docs/modes.md section 4q restated in numpy float64: patch-wise Gram matrices of NHWC features, the layer term,
the loss over the taps, the closed-form gradient, and the first-order error bounds of the fp32 kernels (pesr_amd/csrc/gram.hip).

    G[n, p, c, c'] = s * sum_k F[n, k, c] F[n, k, c'],  s = 1 / (C K)          K = ph pw pixels per patch, P patches per image
    t[n]           = (1 / P) * sum_p sum_cc' (Ga - Gb)^2
    dt/dFa[n, k, c] = g[n] * (4 s / P) * sum_c' dG[n, p(k), c, c'] Fa[n, k, c']  dG = Ga - Gb, symmetric
"""
import numpy as np

U32 = 2.0 ** -24                                                    # the unit roundoff of float32


def patch_of(h, w, patch):
    """0 (the whole map), a side, or (ph, pw) -> (ph, pw)"""
    ph, pw = (patch, patch) if isinstance(patch, int) else patch
    return (ph or h), (pw or w)


def to_patches(f, ph, pw):
    """[N, H, W, C] -> [N, P, K, C], patches row-major, the pixels of a patch row-major"""
    n, h, w, c = f.shape
    assert h % ph == 0 and w % pw == 0
    x = f.reshape(n, h // ph, ph, w // pw, pw, c).transpose(0, 1, 3, 2, 4, 5)
    return x.reshape(n, (h // ph) * (w // pw), ph * pw, c)


def from_patches(x, h, w, ph, pw):
    n, _, _, c = x.shape
    return x.reshape(n, h // ph, w // pw, ph, pw, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)


def gram(f, patch):
    """float64 [N, P, C, C] of the values of f (any float dtype)"""
    ph, pw = patch_of(f.shape[1], f.shape[2], patch)
    x = to_patches(np.asarray(f, dtype=np.float64), ph, pw)
    return np.einsum("npkc,npkd->npcd", x, x) / (f.shape[3] * ph * pw)


def gram_bound(f, patch):
    """Per entry: K products and K additions with one rounding each, in any order, plus the scale:
    (K + 8) 2^-24 s sum_k |F_kc F_kc'|"""
    ph, pw = patch_of(f.shape[1], f.shape[2], patch)
    return (ph * pw + 8) * U32 * gram(np.abs(np.asarray(f, dtype=np.float64)), patch)


def layer(fa, fb, patch):
    """float64 [N]"""
    d = gram(fa, patch) - gram(fb, patch)
    return (d * d).sum(axis=(1, 2, 3)) / d.shape[1]


def grad_from_dg(f, dg, g, patch):
    """g[n] (4 s / P) F dG per patch from a GIVEN dG [N, P, C, C] -> float64 [N, H, W, C]"""
    n, h, w, c = f.shape
    ph, pw = patch_of(h, w, patch)
    x = to_patches(np.asarray(f, dtype=np.float64), ph, pw)
    coef = np.asarray(g, dtype=np.float64) * (4.0 / (c * ph * pw) / x.shape[1])
    out = np.einsum("npkd,npcd->npkc", x, np.asarray(dg, dtype=np.float64)) * coef[:, None, None, None]
    return from_patches(out, h, w, ph, pw)


def grad_bound(f, dg, g, patch):
    """Per element: (C + 8) 2^-24 |g| (4 s / P) sum_c' |dG F|"""
    return (f.shape[3] + 8) * U32 * grad_from_dg(np.abs(np.asarray(f, dtype=np.float64)), np.abs(np.asarray(dg, dtype=np.float64)),
                                                 np.abs(np.asarray(g, dtype=np.float64)), patch)


def layer_grad(fa, fb, g, patch):
    """d(sum_n g[n] t[n]) / dfa, float64 [N, H, W, C]"""
    return grad_from_dg(fa, gram(fa, patch) - gram(fb, patch), g, patch)


def layer_bound(fa, fb, patch):
    """How far the layer term of two fp32 Gram tensors that are each within gram_bound of the exact ones can be from layer(): with
    e = gram_bound(fa) + gram_bound(fb) per entry, |d'^2 - d^2| <= 2 |d| e + e^2; the sum of squares itself is taken in double."""
    d = np.abs(gram(fa, patch) - gram(fb, patch))
    e = gram_bound(fa, patch) + gram_bound(fb, patch)
    return (2.0 * d * e + e * e).sum(axis=(1, 2, 3)) / d.shape[1]


def texture_bound(taps_a, taps_b, patch):
    return sum(layer_bound(fa, fb, patch) for fa, fb in zip(taps_a, taps_b))


def texture(taps_a, taps_b, patch):
    """T[n] = t_1 + t_2 + t_3, the taps in ascending order"""
    total = None
    for fa, fb in zip(taps_a, taps_b):
        t = layer(fa, fb, patch)
        total = t if total is None else total + t
    return total


def features(seed, n, h, w, c):
    """float32 NHWC features with mixed signs and a non-zero mean"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.3, 1.0, (n, h, w, c)) * rng.uniform(0.5, 2.0, (1, 1, 1, c))).astype(np.float32)
