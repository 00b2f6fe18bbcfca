"""NIQE, the no-reference quality score of Mittal et al., as docs/modes.md section 4k restates it in float64.

The image work (luma, crop, the x0.5 scale, both MSCN maps and 26 sums per block and scale) is pesr_amd/csrc/niqe.hip for GPU
tensors (`niqe_stats`) and numpy with the same definition for anything else (`stats_numpy`).  Everything after the sums is host
float64 here: the asymmetric generalised Gaussian (AGGD) fits and the 36 features of a block (`features_from_stats`), the pristine
model (`NiqeModel`, `fit_model`) and the score (`score`, `niqe`).

    python -m pesr_amd.niqe fit --hr_dir DIR --out model.npz [--block 96] [--luma gray]

fits a model from a folder of HR images.  Scores from a self-fitted model compare with each other, not with published tables.
"""
from __future__ import annotations

import math
import os

import numpy as np

# g[k] = exp(-(k-3)^2 / (2 (7/6)^2)) / sum, k = 0..6, the sum taken in ascending k.  niqe.hip carries these doubles as literals.
NIQE_WINDOW = (0.012560200468474614, 0.07882796468173002, 0.2372960771171706, 0.34263151546524945, 0.2372960771171706,
               0.07882796468173002, 0.012560200468474614)
# section 4f's x2-down weights, input index 2*o - 3 + t
DOWN2_WEIGHTS = (-3 / 256, -9 / 256, 29 / 256, 111 / 256, 111 / 256, 29 / 256, -9 / 256, -3 / 256)
LUMA_MODES = {"gray": 0, "y": 1}
GRAY_COEF = (0.298936021293775, 0.587043074451121, 0.114020904255103)
Y_COEF = (65.738 / 256, 129.057 / 256, 25.064 / 256)
NSTAT = 26
NFEAT = 36
SHARPNESS_FRACTION = 0.75


def check_block(block, luma="gray"):
    block = int(block)
    if block < 8 or block > 96 or block % 2:
        raise ValueError(f"niqe: the block side must be even and in 8..96, got {block}")
    if luma not in LUMA_MODES:
        raise ValueError(f"niqe: luma must be one of {sorted(LUMA_MODES)}, got {luma!r}")
    return block


def block_grid(H, W, shave, block):
    """-> (nby, nbx) of an H x W image; ValueError below two blocks (a covariance needs two rows)."""
    shave = int(shave)
    if shave < 0:
        raise ValueError(f"niqe: shave must be >= 0, got {shave}")
    nby, nbx = max(H - 2 * shave, 0) // block, max(W - 2 * shave, 0) // block
    if nby * nbx < 2:
        raise ValueError(f"niqe: a {H} x {W} image with shave {shave} holds {nby * nbx} block(s) of {block} x {block}; at least 2 are needed")
    return nby, nbx


# ---- the device route ----------------------------------------------------------------------------------------------------------
def niqe_stats(t, shave=0, block=96, luma="gray", return_maps=False):
    """[N, 3, H, W] float32 GPU tensor (NCHW-contiguous or channels_last) -> device double [N, 2, nby*nbx, 26]; with return_maps also
    the MSCN maps [N, Hc, Wc] and [N, Hc/2, Wc/2]."""
    import torch

    from . import _lib, ops
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] < 1 or t.shape[1] != 3:
        raise _lib.PesrHipError("niqe_stats: expected a [N, 3, H, W] float32 GPU tensor")
    block = check_block(block, luma)
    N, H, W = t.shape[0], t.shape[2], t.shape[3]
    nby, nbx = block_grid(H, W, shave, block)
    if t.is_contiguous():
        nhwc = 0
    elif t.is_contiguous(memory_format=torch.channels_last):
        nhwc = 1
    else:
        t, nhwc = t.contiguous(), 0
    Hc, Wc = nby * block, nbx * block
    stats = torch.empty((N, 2, nby * nbx, NSTAT), dtype=torch.float64, device=t.device)
    m1 = torch.empty((N, Hc, Wc), dtype=torch.float64, device=t.device) if return_maps else None
    m2 = torch.empty((N, Hc // 2, Wc // 2), dtype=torch.float64, device=t.device) if return_maps else None
    ws = ops.workspace(30 * N * Hc * Wc, t.device)
    rc = _lib.lib().pesr_niqe_stats(t.data_ptr(), N, H, W, nhwc, int(shave), block, LUMA_MODES[luma], stats.data_ptr(),
                                    m1.data_ptr() if return_maps else None, m2.data_ptr() if return_maps else None, ws.data_ptr(),
                                    ws.numel(), ops._stream())
    _lib.check(rc, "pesr_niqe_stats")
    return (stats, m1, m2) if return_maps else stats


# ---- the numpy route: the same definition, for CPU tensors and arrays -------------------------------------------------------------
def _as_chw(img):
    a = img.detach().cpu().numpy() if hasattr(img, "detach") else np.asarray(img)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"niqe: expected a [1, 3, H, W] or [3, H, W] image, got {tuple(a.shape)}")
    return a


def luma_image(img, mode="gray"):
    """[3, H, W] of 0..255 floats -> the integer-valued float64 luma [H, W]."""
    rgb = np.rint(np.clip(np.asarray(img).astype(np.float64), 0.0, 255.0))
    if mode == "gray":
        return np.floor(((rgb[0] * GRAY_COEF[0] + rgb[1] * GRAY_COEF[1]) + rgb[2] * GRAY_COEF[2]) + 0.5)
    y = ((rgb[0] * Y_COEF[0] + rgb[1] * Y_COEF[1]) + rgb[2] * Y_COEF[2]) + 16.0
    return np.rint(np.clip(y, 0.0, 255.0))


def _reflect_index(j, n):
    m = np.mod(j, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _down2_axis0(a):
    o = np.arange(a.shape[0] // 2)
    acc = np.zeros((a.shape[0] // 2,) + a.shape[1:])
    for t in range(8):
        acc = acc + DOWN2_WEIGHTS[t] * a[_reflect_index(2 * o - 3 + t, a.shape[0])]
    return acc


def down2(a):
    """x0.5 antialiased bicubic of a float64 image with even sides: height pass, then width pass, nothing rounded or clamped."""
    return np.ascontiguousarray(_down2_axis0(_down2_axis0(a).T).T)


def _filter(a):
    """The 7-tap window along the height, then along the width, "same" size, edges replicated."""
    h, w = a.shape
    p = np.pad(a, ((3, 3), (0, 0)), mode="edge")
    acc = np.zeros((h, w))
    for k in range(7):
        acc = acc + NIQE_WINDOW[k] * p[k:k + h, :]
    p = np.pad(acc, ((0, 0), (3, 3)), mode="edge")
    out = np.zeros((h, w))
    for k in range(7):
        out = out + NIQE_WINDOW[k] * p[:, k:k + w]
    return out


def mscn(a):
    """float64 image -> (MSCN map, sigma map)."""
    mu = _filter(a)
    sigma = np.sqrt(np.abs(_filter(a * a) - mu * mu))
    return (a - mu) / (sigma + 1.0), sigma


def _block_stats(m, sigma, bs):
    nby, nbx = m.shape[0] // bs, m.shape[1] // bs
    blk = m.reshape(nby, bs, nbx, bs).transpose(0, 2, 1, 3)                       # [nby, nbx, bs, bs]
    out = np.empty((nby, nbx, NSTAT))
    for q, d in enumerate((None, (0, 1), (1, 0), (1, 1), (1, -1))):
        x = blk if d is None else blk * np.roll(blk, d, axis=(2, 3))              # the shift wraps inside the block
        xx = x * x
        neg, pos = x < 0, x > 0
        out[..., 5 * q] = np.where(neg, xx, 0.0).sum(axis=(2, 3))
        out[..., 5 * q + 1] = neg.sum(axis=(2, 3))
        out[..., 5 * q + 2] = np.where(pos, xx, 0.0).sum(axis=(2, 3))
        out[..., 5 * q + 3] = pos.sum(axis=(2, 3))
        out[..., 5 * q + 4] = np.abs(x).sum(axis=(2, 3))
    out[..., 25] = sigma.reshape(nby, bs, nbx, bs).sum(axis=(1, 3))
    return out.reshape(nby * nbx, NSTAT)


def stats_numpy(img, shave=0, block=96, luma="gray", return_maps=False):
    """One image ([1, 3, H, W] / [3, H, W] tensor or array) -> float64 [2, nby*nbx, 26], what niqe_stats gives for it."""
    a = _as_chw(img)
    block = check_block(block, luma)
    H, W = a.shape[1], a.shape[2]
    nby, nbx = block_grid(H, W, shave, block)
    shave = int(shave)
    i1 = luma_image(a, luma)[shave:shave + nby * block, shave:shave + nbx * block]
    m1, s1 = mscn(i1)
    m2, s2 = mscn(down2(i1))
    stats = np.stack([_block_stats(m1, s1, block), _block_stats(m2, s2, block // 2)])
    return (stats, m1, m2) if return_maps else stats


# ---- features -------------------------------------------------------------------------------------------------------------------
_TABLE = None


def alpha_table():
    """The AGGD shape grid a = (200 + i) / 1000, i = 0..9800, with r(a) = gamma(2/a)^2 / (gamma(1/a) gamma(3/a)), sqrt(gamma(1/a) /
    gamma(3/a)) and gamma(2/a) / gamma(1/a); built once."""
    global _TABLE
    if _TABLE is None:
        a = np.array([(200 + i) / 1000 for i in range(9801)])
        g1 = np.array([math.gamma(1 / v) for v in a])
        g2 = np.array([math.gamma(2 / v) for v in a])
        g3 = np.array([math.gamma(3 / v) for v in a])
        _TABLE = (a, (g2 * g2) / (g1 * g3), np.sqrt(g1 / g3), g2 / g1)
    return _TABLE


def aggd_fit(five, n):
    """[M, 5] sums {L2, nl, R2, nr, A} of maps of n values -> (grid index [M], alpha, bl, br, mean), each [M]; non-finite (index -1) where a side
    is empty.  alpha is the FIRST minimiser of (r(a) - rn)^2 over the grid."""
    a, r, sq, g21 = alpha_table()
    five = np.asarray(five, dtype=np.float64).reshape(-1, 5)
    L2, nl, R2, nr, A = (five[:, k] for k in range(5))
    with np.errstate(all="ignore"):
        ls, rs = np.sqrt(L2 / nl), np.sqrt(R2 / nr)
        gh = ls / rs
        rhat = ((A / n) * (A / n)) / ((L2 + R2) / n)
        gh2 = gh * gh
        rn = rhat * (gh2 * gh + 1.0) * (gh + 1.0) / ((gh2 + 1.0) * (gh2 + 1.0))
        ok = np.isfinite(rn) & np.isfinite(ls) & np.isfinite(rs) & (nl > 0) & (nr > 0)
        idx = np.zeros(len(rn), dtype=np.int64)
        for lo in range(0, len(rn), 256):
            d = r[None, :] - np.where(ok[lo:lo + 256], rn[lo:lo + 256], 0.0)[:, None]
            idx[lo:lo + 256] = np.argmin(d * d, axis=1)
        nan = np.where(ok, 0.0, np.nan)
        alpha = a[idx] + nan
        bl, br = ls * sq[idx] + nan, rs * sq[idx] + nan
        mean = (br - bl) * g21[idx]
    return np.where(ok, idx, -1), alpha, bl, br, mean


def features_from_stats(stats, block, return_index=False):
    """[..., 2, nblk, 26] block sums (device tensor or array) -> float64 [..., nblk, 36]: per scale [alpha, (bl+br)/2] of the MSCN
    map and [alpha, mean, bl, br] of each of the four product maps.  A block with an empty side in any map has a non-finite row."""
    s = stats.detach().cpu().numpy() if hasattr(stats, "detach") else np.asarray(stats, dtype=np.float64)
    if s.ndim < 3 or s.shape[-3] != 2 or s.shape[-1] != NSTAT:
        raise ValueError(f"niqe: expected [..., 2, blocks, 26] block sums, got {tuple(s.shape)}")
    lead, nblk = s.shape[:-3], s.shape[-2]
    s = s.reshape((-1, 2, nblk, NSTAT))
    feat = np.empty((s.shape[0], nblk, NFEAT))
    index = np.empty((s.shape[0], nblk, 10), dtype=np.int64)
    for sc in range(2):
        n = float((block >> sc) * (block >> sc))
        col = 18 * sc
        for q in range(5):
            idx, alpha, bl, br, mean = aggd_fit(s[:, sc, :, 5 * q:5 * q + 5], n)
            index[:, :, 5 * sc + q] = idx.reshape(-1, nblk)
            parts = (alpha, (bl + br) / 2) if q == 0 else (alpha, mean, bl, br)
            for v in parts:
                feat[:, :, col] = v.reshape(-1, nblk)
                col += 1
    feat = feat.reshape(lead + (nblk, NFEAT))
    return (feat, index.reshape(lead + (nblk, 10))) if return_index else feat


def _finite_rows(feat, name):
    keep = np.isfinite(feat).all(axis=1)
    if int(keep.sum()) < 2:
        raise ValueError(f"niqe: {name}: {int(keep.sum())} of {len(feat)} blocks have finite features (a map without values on both "
                         "sides of zero, as a constant block gives, has none); at least 2 are needed")
    return feat[keep]


# ---- the model and the score ----------------------------------------------------------------------------------------------------
class NiqeModel:
    """Mean and covariance of the features of the sharp blocks of a set of pristine images, with the block side and luma they were
    taken with."""

    def __init__(self, mu, cov, block=96, luma="gray", rows=0):
        self.mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1))
        self.cov = np.ascontiguousarray(np.asarray(cov, dtype=np.float64))
        self.block = check_block(block, luma)
        self.luma = str(luma)
        self.rows = int(rows)
        if self.mu.shape != (NFEAT,) or self.cov.shape != (NFEAT, NFEAT):
            raise ValueError(f"niqe model: mu must hold {NFEAT} values and cov {NFEAT} x {NFEAT}, got {self.mu.shape} and {self.cov.shape}")
        if not (np.isfinite(self.mu).all() and np.isfinite(self.cov).all()):
            raise ValueError("niqe model: non-finite mu or cov")

    def save(self, path):
        with open(path, "wb") as fh:                                 # (a file object: numpy appends no suffix)
            np.savez(fh, mu=self.mu, cov=self.cov, block=np.int64(self.block), luma=np.array(self.luma), rows=np.int64(self.rows))

    @staticmethod
    def load(path):
        """.npz written by save(), or a .mat holding mu_prisparam and cov_prisparam (the standard pristine model: block 96, luma
        "gray"), which needs scipy.  ValueError with the reason otherwise."""
        if not os.path.isfile(path):
            raise ValueError(f"{path}: no such file")
        if str(path).lower().endswith(".mat"):
            try:
                import scipy.io
            except ImportError:
                raise ValueError(f"{path}: a .mat model is read with scipy.io, and scipy is not installed; fit a .npz model with "
                                 "`python -m pesr_amd.niqe fit`") from None
            try:
                d = scipy.io.loadmat(path)
                return NiqeModel(d["mu_prisparam"], d["cov_prisparam"], 96, "gray", 0)
            except Exception as e:
                raise ValueError(f"{path}: not a NIQE model (.mat with mu_prisparam and cov_prisparam): {e}") from None
        try:
            with np.load(path, allow_pickle=False) as d:
                return NiqeModel(d["mu"], d["cov"], int(d["block"]), str(d["luma"]), int(d["rows"]))
        except Exception as e:
            raise ValueError(f"{path}: not a NIQE model (.npz with mu, cov, block, luma, rows): {e}") from None


def load_model_flag(prog, flag, path):
    """Entry points: the model named by `flag`, or SystemExit naming the program and the flag.  No GPU is touched."""
    try:
        return NiqeModel.load(path)
    except ValueError as e:
        raise SystemExit(f"{prog}: {flag} {e}")


def check_fits_flag(prog, flags, model, H, W, shave, name):
    """SystemExit unless an H x W image with `shave` holds the model's block twice."""
    try:
        block_grid(H, W, shave, model.block)
    except ValueError as e:
        raise SystemExit(f"{prog}: {flags}: {name}: {e}")


def score(feat, model, name="image"):
    """[nblk, 36] features of one image -> NIQE against the model; rows with a non-finite value are dropped from mean and covariance."""
    f = _finite_rows(np.asarray(feat, dtype=np.float64), name)
    d = model.mu - f.mean(axis=0)
    c = (model.cov + np.cov(f, rowvar=False)) / 2.0
    return float(np.sqrt(d @ np.linalg.pinv(c) @ d))


def _is_gpu_batch(t):
    try:
        import torch
    except ImportError:                                             # pragma: no cover
        return False
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3


def image_stats(t, shave, block, luma):
    """float32 GPU [N, 3, H, W] -> the kernel; anything else is one image for the numpy route.  -> float64 array [N, 2, nblk, 26]."""
    if _is_gpu_batch(t):
        return niqe_stats(t.detach(), shave, block, luma).cpu().numpy()
    return stats_numpy(t, shave, block, luma)[None]


def niqe(t, model, shave=0, names=None):
    """NIQE of every image of `t` against `model` -> list of floats."""
    s = image_stats(t, shave, model.block, model.luma)
    feat = features_from_stats(s, model.block)
    return [score(feat[i], model, names[i] if names else f"image {i}") for i in range(len(feat))]


def fit_model(images, block=96, luma="gray"):
    """Pristine model from HR images (an iterable of [1, 3, H, W] / [3, H, W] images; float32 GPU tensors go through the kernel): per
    image the blocks whose scale-1 sharpness (mean sigma) exceeds 0.75 of that image's largest, their feature rows stacked."""
    block = check_block(block, luma)
    rows = []
    for k, img in enumerate(images):
        s = image_stats(img, 0, block, luma)
        feat = features_from_stats(s, block)
        for i in range(len(s)):
            sharp = s[i, 0, :, 25] / float(block * block)
            rows.append(feat[i][sharp > SHARPNESS_FRACTION * sharp.max()])
    if not rows:
        raise ValueError("niqe fit: no images")
    f = _finite_rows(np.concatenate(rows), "the fitting set")
    return NiqeModel(f.mean(axis=0), np.cov(f, rowvar=False), block, luma, len(f))


def main(argv=None):
    import argparse
    import glob
    parser = argparse.ArgumentParser(prog="python -m pesr_amd.niqe", description="fit a NIQE pristine model from a folder of HR images")
    sub = parser.add_subparsers(dest="cmd", required=True)
    fit = sub.add_parser("fit")
    fit.add_argument("--hr_dir", required=True, help="folder of HR PNGs")
    fit.add_argument("--out", required=True, help="the model file to write (.npz)")
    fit.add_argument("--block", type=int, default=96)
    fit.add_argument("--luma", default="gray", choices=sorted(LUMA_MODES))
    args = parser.parse_args(argv)
    try:
        check_block(args.block, args.luma)
    except ValueError as e:
        raise SystemExit(f"niqe fit: --block: {e}")
    paths = sorted(glob.glob(os.path.join(args.hr_dir, "*.png")))
    if not paths:
        raise SystemExit(f"niqe fit: --hr_dir {args.hr_dir}: no PNG files")
    import torch
    from PIL import Image
    device = torch.device("cuda") if torch.cuda.is_available() else None

    def images():
        for p in paths:
            a = np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB")).transpose(2, 0, 1)).astype(np.float32)
            yield torch.from_numpy(a)[None].to(device) if device is not None else a
    try:
        model = fit_model(images(), args.block, args.luma)
    except ValueError as e:
        raise SystemExit(f"niqe fit: {e}")
    model.save(args.out)
    print(f"{args.out}: {model.rows} blocks of {model.block} x {model.block} from {len(paths)} image(s), luma {model.luma}")


if __name__ == "__main__":
    main()
