"""The classical degradation model on the device, LR = (HR (*) k) subsampled by s, plus noise, as pinned in docs/modes.md section 4j:
a K x K float64 blur kernel centred on the s x s block of every LR pixel (where the bicubic LR pixel of section 4f sits), replicate
clamp at the image border, a twelve-term Irwin-Hall noise made from integers, clamp to [0, 255], round half up.  Kernel:
csrc/degrade.hip.  The blur kernels are made here, on the host, in float64; the device never evaluates exp.
The steps that may follow it - the resize jitter of section 4m, the JPEG round trip of section 4l - are chained here too, in
degrade_chain_pool_u8 (n windows of a pool: the training sampler) and lr_image_u8 (one whole image: test.py, train.py's validation).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _pool
from .resize import METHODS, imresize_to_pool_u8, imresize_u8

SCALES = (2, 3, 4)
MAX_K = 24
DESC_WORDS = 11            # int64 words per descriptor row (include/pesr_hip.h)


def legal_kernel_size(s: int, K: int) -> bool:
    return 1 <= K <= MAX_K and (K - s) % 2 == 0


def kernel_size(s: int, sigma_hi: float) -> int:
    """The smallest legal K (1 <= K <= 24, K of the parity of s) with K >= 6 * sigma_hi, capped at the largest legal one."""
    if s not in SCALES:
        raise ValueError(f"degradation: factor {s} is not supported (2, 3, 4)")
    K = max(1, int(math.ceil(6.0 * sigma_hi)))
    if (K - s) % 2:
        K += 1
    return min(K, MAX_K if s % 2 == 0 else MAX_K - 1)


def gaussian_kernel(K: int, sigma1: float, sigma2: Optional[float] = None, theta: float = 0.0) -> np.ndarray:
    """float64 [K][K]: w[i][j] = exp(-0.5 (a u^2 + 2 b u v + c v^2)), u = j - (K-1)/2, v = i - (K-1)/2, [[a, b], [b, c]] the inverse
    of R(theta) diag(sigma1^2, sigma2^2) R(theta)^T, divided by the sum taken in row-major order.  Host only."""
    sigma2 = sigma1 if sigma2 is None else sigma2
    if not (K >= 1 and sigma1 > 0 and sigma2 > 0):
        raise ValueError(f"gaussian_kernel: K = {K}, sigma = ({sigma1}, {sigma2}): K >= 1 and positive sigmas expected")
    ct, st = math.cos(theta), math.sin(theta)
    i1, i2 = 1.0 / (sigma1 * sigma1), 1.0 / (sigma2 * sigma2)
    a = ct * ct * i1 + st * st * i2
    b = ct * st * (i1 - i2)
    c = st * st * i1 + ct * ct * i2
    t = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    u, v = t[None, :], t[:, None]
    w = np.exp(-0.5 * (a * (u * u) + (2.0 * b) * (u * v) + c * (v * v)))
    total = np.cumsum(w.reshape(-1))[-1]            # (cumsum adds strictly left to right)
    return w / total


def delta_kernel(s: int) -> np.ndarray:
    """The narrowest legal kernel, equal weights: the centre pixel of the block at x3, the mean of its four central pixels at x2 and
    x4 - "no blur" on the LR grid of section 4f."""
    K = kernel_size(s, 0.0)
    return np.full((K, K), 1.0 / (K * K), dtype=np.float64)


def degrade_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], s: int, kernels, kernel_index: Sequence[int],
                    noise_sigma: Sequence[float], noise_stream: Sequence[int], windows: Optional[Sequence[Tuple[int, int, int, int]]] = None):
    """Degrade windows of the images of a flat device-resident uint8 pool (image of entry i: HWC bytes at offsets[i], shapes[i] =
    (H, W), both multiples of s) in ONE launch.  kernels: float64 [n_kernels][K][K]; entry i uses kernels[kernel_index[i]], noise
    level noise_sigma[i] and noise stream noise_stream[i]; windows[i] = (y0, x0, h, w) in the image's LR grid, None = every whole
    image.  Several entries may name the same image.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    _pool.check_pool(pool, "degrade_pool_u8")
    n = len(offsets)
    assert n > 0 and n == len(shapes) == len(kernel_index) == len(noise_sigma) == len(noise_stream)
    bank = np.ascontiguousarray(np.asarray(kernels, dtype=np.float64))
    assert bank.ndim == 3 and bank.shape[1] == bank.shape[2], "kernels: [n_kernels][K][K] expected"
    K = int(bank.shape[1])
    if s not in SCALES:
        raise _lib.PesrHipError(f"degrade: factor {s} is not supported (2, 3, 4)")
    if not legal_kernel_size(s, K):
        raise _lib.PesrHipError(f"degrade: a {K} x {K} kernel is not legal at x{s}: 1 <= K <= {MAX_K} of the parity of the factor")
    if windows is None:
        windows = [(0, 0, h // s, w // s) for h, w in shapes]
    assert len(windows) == n
    desc = np.empty((n, DESC_WORDS), dtype=np.int64)
    out_off = 0
    for i in range(n):
        (H, W), (y0, x0, h, w) = shapes[i], windows[i]
        assert 0 <= offsets[i] and offsets[i] + 3 * H * W <= pool.numel(), "image outside the pool"
        if H < 1 or W < 1 or H % s or W % s:
            raise _lib.PesrHipError(f"degrade: a {H} x {W} image cannot be reduced by {s}: mod-crop it first (modcrop)")
        desc[i] = (int(offsets[i]), out_off, H, W, y0, x0, h, w, int(kernel_index[i]), _pool.f64_bits(noise_sigma[i]), _pool.i64(int(noise_stream[i])))
        out_off += 3 * max(h, 0) * max(w, 0)
    dev = pool.device
    out = torch.empty(max(out_off, 1), dtype=torch.uint8, device=dev)
    bank_dev = torch.from_numpy(bank).to(dev)
    _pool.launch("pesr_degrade_u8", pool, out, desc, int(s), K, bank_dev.data_ptr(), int(bank.shape[0]))
    return out[:out_off], [int(v) for v in desc[:, 1]], [(int(wd[2]), int(wd[3])) for wd in windows]


def degrade_u8(img: torch.Tensor, s: int, kernel, noise_sigma: float = 0.0, noise_stream: int = 0) -> torch.Tensor:
    """uint8 HWC device tensor (sides multiples of s) -> its uint8 HWC LR image, sides divided by s."""
    flat, h, w = _pool.image_as_pool(img, "degrade_u8")
    out, _, [(ho, wo)] = degrade_pool_u8(flat, [0], [(h, w)], s, np.asarray(kernel, dtype=np.float64)[None], [0],
                                         [noise_sigma], [noise_stream])
    return out.view(ho, wo, 3)


class _BlurNoise(NamedTuple):
    sigma_lo: float
    sigma_hi: float
    aniso: bool = False
    noise_hi: float = 0.0


class DegradationSpec(_BlurNoise):
    """The ranges a blind-training sample's degradation is drawn from: blur sigma in [sigma_lo, sigma_hi] (HR pixels), a second
    sigma and an angle when `aniso`, a noise level in [0, noise_hi] (grey levels) when noise_hi > 0, a JPEG quality in
    jpeg_lo .. jpeg_hi (docs/modes.md section 4l; 4:2:0 chroma unless `jpeg_420` is false) when jpeg_hi > 0, a resize jitter
    (section 4m: a round trip through an intermediate size of r times the sides, r in [jitter_lo, jitter_hi], with a random filter
    each way) when jitter_hi > 0.  As a tuple it is the four blur and noise values, as it was before JPEG; jpeg_lo, jpeg_hi,
    jpeg_420, jitter_lo and jitter_hi are trailing constructor arguments with defaults and plain attributes."""

    def __new__(cls, sigma_lo, sigma_hi, aniso=False, noise_hi=0.0, jpeg_lo=0, jpeg_hi=0, jpeg_420=True, jitter_lo=0.0, jitter_hi=0.0):
        self = super().__new__(cls, sigma_lo, sigma_hi, aniso, noise_hi)
        self.jpeg_lo, self.jpeg_hi, self.jpeg_420 = int(jpeg_lo), int(jpeg_hi), bool(jpeg_420)
        self.jitter_lo, self.jitter_hi = float(jitter_lo), float(jitter_hi)
        return self

    def __repr__(self):
        return f"DegradationSpec{tuple(self) + (self.jpeg_lo, self.jpeg_hi, self.jpeg_420, self.jitter_lo, self.jitter_hi)!r}"

    def fields(self):
        """The names of the values draw() returns, in its order: what is at which position depends on the spec."""
        names = ("sigma1", "sigma2", "theta", "sigma_n", "q")
        if self.jpeg_hi:
            names += ("jpeg_quality",)
        if self.jitter_hi:
            names += ("jitter_r", "jitter_m1", "jitter_m2")
        return names

    def named(self, drawn):
        """A drawn tuple (or the tail of a sampler's pick that holds one) as a dict by field name."""
        names = self.fields()
        assert len(drawn) == len(names), (len(drawn), names)
        return dict(zip(names, drawn))

    def draw(self, rng):
        """-> (sigma1, sigma2, theta, sigma_n, q) from `rng` (a random.Random) alone, in this fixed order: sigma1; if aniso, sigma2 in
        [sigma_lo, sigma1], then theta in [0, pi); if noise_hi > 0, sigma_n; always q = 64 random bits; if jpeg_hi > 0, a sixth value
        after q: the JPEG quality, an integer in jpeg_lo .. jpeg_hi; if jitter_hi > 0, three more after everything else: r in
        [jitter_lo, jitter_hi] and the two filters, indices into pesr_amd.resize.METHODS.  fields() names what was drawn."""
        sigma1 = rng.uniform(self.sigma_lo, self.sigma_hi)
        sigma2, theta, sigma_n = sigma1, 0.0, 0.0
        if self.aniso:
            sigma2 = rng.uniform(self.sigma_lo, sigma1)
            theta = rng.uniform(0.0, math.pi)
        if self.noise_hi > 0:
            sigma_n = rng.uniform(0.0, self.noise_hi)
        drawn = (sigma1, sigma2, theta, sigma_n, rng.getrandbits(64))
        if self.jpeg_hi:
            drawn += (rng.randint(self.jpeg_lo, self.jpeg_hi),)
        if self.jitter_hi:
            drawn += (rng.uniform(self.jitter_lo, self.jitter_hi), rng.randrange(3), rng.randrange(3))
        return drawn

    def check(self, who: str = "DegradationSpec"):
        if not (0 < self.sigma_lo <= self.sigma_hi and math.isfinite(self.sigma_hi)):
            raise SystemExit(f"{who}: the blur range {self.sigma_lo},{self.sigma_hi} must be 0 < LO <= HI")
        if not (self.noise_hi >= 0 and math.isfinite(self.noise_hi)):
            raise SystemExit(f"{who}: the noise level {self.noise_hi} must be >= 0")
        if (self.jpeg_lo or self.jpeg_hi) and not 1 <= self.jpeg_lo <= self.jpeg_hi <= 100:
            raise SystemExit(f"{who}: the JPEG quality range {self.jpeg_lo},{self.jpeg_hi} must be 1 <= LO <= HI <= 100")
        if (self.jitter_lo or self.jitter_hi) and not 0.125 <= self.jitter_lo <= self.jitter_hi <= 8:
            raise SystemExit(f"{who}: the resize-jitter range {self.jitter_lo},{self.jitter_hi} must be 0.125 <= LO <= HI <= 8")
        return self


def jitter_size(n: int, r: float) -> int:
    """Q(n) = min(8n, max(ceil(n / 8), floor(r n + 0.5))): the intermediate length of the resize jitter, kept inside section 4m's limits."""
    return min(8 * n, max(-(-n // 8), int(math.floor(r * n + 0.5))))


def resize_jitter_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], r: Sequence[float],
                          m1: Sequence[int], m2: Sequence[int], noise_sigma=None, noise_stream=None, strides=None):
    """The resize-jitter round trip of docs/modes.md section 4m for n windows of a device-resident uint8 pool: entry i goes from
    h x w to Q(h) x Q(w) with filter METHODS[m1[i]] and back to h x w with METHODS[m2[i]], the noise in the second resize's width
    pass: two pooled resizes, four launches.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    mids = [(jitter_size(h, ri), jitter_size(w, ri)) for (h, w), ri in zip(shapes, r)]
    mid, mid_off, _ = imresize_to_pool_u8(pool, offsets, shapes, mids, [METHODS[i] for i in m1], strides=strides)
    return imresize_to_pool_u8(mid, mid_off, mids, shapes, [METHODS[i] for i in m2], noise_sigma=noise_sigma, noise_stream=noise_stream)


def resize_jitter_u8(img: torch.Tensor, r: float, m1: int = 0, m2: int = 0, noise_sigma: float = 0.0, noise_stream: int = 0) -> torch.Tensor:
    """uint8 HWC device tensor -> the same size, after the resize-jitter round trip through Q(h) x Q(w)."""
    flat, h, w = _pool.image_as_pool(img, "resize_jitter_u8")
    out, _, _ = resize_jitter_pool_u8(flat, [0], [(h, w)], [r], [m1], [m2], [noise_sigma], [noise_stream])
    return out.view(h, w, 3)


def degrade_chain_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], s: int, kernels, kernel_index: Sequence[int],
                          noise_sigma: Sequence[float], noise_stream: Sequence[int], windows=None, jitter=None, jpeg=None, jpeg_420: bool = True):
    """The whole degradation of n windows, in its one order: degrade_pool_u8 (blur, subsample, noise); with jitter = (r, m1, m2), a
    list per entry each, resize_jitter_pool_u8, and the noise moves out of the degrade launch into the jitter's second resize; with
    jpeg = a quality per entry, jpeg_pool_u8 last, in place on the chain's own scratch pool (4:2:0 chroma unless jpeg_420 is
    false).  The other arguments are degrade_pool_u8's.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    out, offs, out_shapes = degrade_pool_u8(pool, offsets, shapes, s, kernels, kernel_index, [0.0] * len(offsets) if jitter else noise_sigma,
                                            noise_stream, windows)
    if jitter:
        out, offs, out_shapes = resize_jitter_pool_u8(out, offs, out_shapes, jitter[0], jitter[1], jitter[2], noise_sigma, noise_stream)
    if jpeg:
        from .jpeg import jpeg_pool_u8
        jpeg_pool_u8(out, offs, out_shapes, [w for _, w in out_shapes], jpeg, jpeg_420, out=out)
    return out, offs, out_shapes


def lr_image_u8(hr: torch.Tensor, s: int, kernel=None, noise_sigma: float = 0.0, noise_stream: int = 0, jitter=None, jpeg_q: int = 0,
                jpeg_420: bool = True) -> torch.Tensor:
    """uint8 HWC device tensor (sides multiples of s) -> its uint8 HWC LR image.  kernel None: the bicubic resize of section 4f, then
    the JPEG round trip when jpeg_q; a blur kernel: the chain above for this one image, jitter = (r, m1, m2)."""
    if kernel is None:
        lr = imresize_u8(hr, s, up=False)
        if jpeg_q:
            from .jpeg import jpeg_u8
            lr = jpeg_u8(lr, jpeg_q, jpeg_420)
        return lr
    flat, h, w = _pool.image_as_pool(hr, "lr_image_u8")
    out, _, [(ho, wo)] = degrade_chain_pool_u8(flat, [0], [(h, w)], s, np.asarray(kernel, dtype=np.float64)[None], [0], [noise_sigma], [noise_stream],
                                               jitter=[[v] for v in jitter] if jitter else None, jpeg=[jpeg_q] if jpeg_q else None, jpeg_420=jpeg_420)
    return out.view(ho, wo, 3)


def parse_resize_jitter(text: str, who: str):
    """test.py's 'R[,M1[,M2]]' -> (r, m1, m2), the filters as indices into pesr_amd.resize.METHODS (default bicubic); SystemExit
    naming the flag for a bad number, a ratio outside 0.125 .. 8 or an unknown filter name."""
    parts = str(text).split(",")
    try:
        r = float(parts[0])
    except ValueError:
        raise SystemExit(f"{who}: --resize_jitter {text!r}: R[,M1[,M2]] expected, R a number")
    if not (0.125 <= r <= 8) or len(parts) > 3:
        raise SystemExit(f"{who}: --resize_jitter {text!r}: R[,M1[,M2]] expected, 0.125 <= R <= 8")
    names = parts[1:] + ["bicubic"] * (3 - len(parts))
    for m in names:
        if m not in METHODS:
            raise SystemExit(f"{who}: --resize_jitter {text!r}: filter {m!r} is not one of {', '.join(METHODS)}")
    return r, METHODS.index(names[0]), METHODS.index(names[1])


def parse_sigma_list(text: str, who: str, flag: str, counts: Sequence[int]):
    """'A,B,...' -> floats; SystemExit naming the flag when a field is no number or the count is not one of `counts`."""
    try:
        vals = [float(t) for t in str(text).split(",")]
    except ValueError:
        raise SystemExit(f"{who}: {flag} {text!r}: comma-separated numbers expected")
    if len(vals) not in counts:
        raise SystemExit(f"{who}: {flag} {text!r}: {' or '.join(str(c) for c in counts)} value(s) expected")
    return vals
