"""The classical degradation model on the device, LR = (HR (*) k) subsampled by s, plus noise, as pinned in docs/modes.md section 4j:
a K x K float64 blur kernel centred on the s x s block of every LR pixel (where the bicubic LR pixel of section 4f sits), replicate
clamp at the image border, a twelve-term Irwin-Hall noise made from integers, clamp to [0, 255], round half up.  Kernel:
csrc/degrade.hip.  The blur kernels are made here, on the host, in float64; the device never evaluates exp.
"""
from __future__ import annotations

import ctypes
import math
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SCALES = (2, 3, 4)
MAX_K = 24
DESC_WORDS = 11            # int64 words per descriptor row (include/pesr_hip.h)
_MASK = (1 << 64) - 1


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


def _f64_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _i64(q: int) -> int:
    q &= _MASK
    return q - (1 << 64) if q >> 63 else q


def degrade_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], s: int, kernels, kernel_index: Sequence[int],
                    noise_sigma: Sequence[float], noise_stream: Sequence[int], windows: Optional[Sequence[Tuple[int, int, int, int]]] = None):
    """Degrade windows of the images of a flat device-resident uint8 pool (image of entry i: HWC bytes at offsets[i], shapes[i] =
    (H, W), both multiples of s) in ONE launch.  kernels: float64 [n_kernels][K][K]; entry i uses kernels[kernel_index[i]], noise
    level noise_sigma[i] and noise stream noise_stream[i]; windows[i] = (y0, x0, h, w) in the image's LR grid, None = every whole
    image.  Several entries may name the same image.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    if not (torch.is_tensor(pool) and pool.is_cuda):
        raise _lib.PesrHipError("degrade_pool_u8 needs a device tensor: pesr_amd has no CPU fallback")
    assert pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()
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
        desc[i] = (int(offsets[i]), out_off, H, W, y0, x0, h, w, int(kernel_index[i]), _f64_bits(noise_sigma[i]), _i64(int(noise_stream[i])))
        out_off += 3 * max(h, 0) * max(w, 0)
    dev = pool.device
    out = torch.empty(max(out_off, 1), dtype=torch.uint8, device=dev)
    bank_dev = torch.from_numpy(bank).to(dev)
    desc_dev = torch.from_numpy(desc).to(dev)              # the library checks the host copy; the kernel reads this one
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().pesr_degrade_u8(pool.data_ptr(), out.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), desc_dev.data_ptr(), n, int(s),
                                          K, bank_dev.data_ptr(), int(bank.shape[0]), stream), "pesr_degrade_u8")
    return out[:out_off], [int(v) for v in desc[:, 1]], [(int(wd[2]), int(wd[3])) for wd in windows]


def degrade_u8(img: torch.Tensor, s: int, kernel, noise_sigma: float = 0.0, noise_stream: int = 0) -> torch.Tensor:
    """uint8 HWC device tensor (sides multiples of s) -> its uint8 HWC LR image, sides divided by s."""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise _lib.PesrHipError("degrade_u8 needs a device tensor: pesr_amd has no CPU fallback")
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, "uint8 [H][W][3] expected"
    h, w = int(img.shape[0]), int(img.shape[1])
    out, _, [(ho, wo)] = degrade_pool_u8(img.contiguous().view(-1), [0], [(h, w)], s, np.asarray(kernel, dtype=np.float64)[None], [0],
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
    jpeg_lo .. jpeg_hi (docs/modes.md section 4l; 4:2:0 chroma unless `jpeg_420` is false) when jpeg_hi > 0.  As a tuple it is the
    four blur and noise values, as it was before JPEG; jpeg_lo, jpeg_hi and jpeg_420 are trailing constructor arguments with
    defaults and plain attributes."""

    def __new__(cls, sigma_lo, sigma_hi, aniso=False, noise_hi=0.0, jpeg_lo=0, jpeg_hi=0, jpeg_420=True):
        self = super().__new__(cls, sigma_lo, sigma_hi, aniso, noise_hi)
        self.jpeg_lo, self.jpeg_hi, self.jpeg_420 = int(jpeg_lo), int(jpeg_hi), bool(jpeg_420)
        return self

    def __repr__(self):
        return f"DegradationSpec{tuple(self) + (self.jpeg_lo, self.jpeg_hi, self.jpeg_420)!r}"

    def draw(self, rng):
        """-> (sigma1, sigma2, theta, sigma_n, q) from `rng` (a random.Random) alone, in this fixed order: sigma1; if aniso, sigma2 in
        [sigma_lo, sigma1], then theta in [0, pi); if noise_hi > 0, sigma_n; always q = 64 random bits; if jpeg_hi > 0, a sixth value
        after q: the JPEG quality, an integer in jpeg_lo .. jpeg_hi."""
        sigma1 = rng.uniform(self.sigma_lo, self.sigma_hi)
        sigma2, theta, sigma_n = sigma1, 0.0, 0.0
        if self.aniso:
            sigma2 = rng.uniform(self.sigma_lo, sigma1)
            theta = rng.uniform(0.0, math.pi)
        if self.noise_hi > 0:
            sigma_n = rng.uniform(0.0, self.noise_hi)
        drawn = (sigma1, sigma2, theta, sigma_n, rng.getrandbits(64))
        return drawn + (rng.randint(self.jpeg_lo, self.jpeg_hi),) if self.jpeg_hi else drawn

    def check(self, who: str = "DegradationSpec"):
        if not (0 < self.sigma_lo <= self.sigma_hi and math.isfinite(self.sigma_hi)):
            raise SystemExit(f"{who}: the blur range {self.sigma_lo},{self.sigma_hi} must be 0 < LO <= HI")
        if not (self.noise_hi >= 0 and math.isfinite(self.noise_hi)):
            raise SystemExit(f"{who}: the noise level {self.noise_hi} must be >= 0")
        if (self.jpeg_lo or self.jpeg_hi) and not 1 <= self.jpeg_lo <= self.jpeg_hi <= 100:
            raise SystemExit(f"{who}: the JPEG quality range {self.jpeg_lo},{self.jpeg_hi} must be 1 <= LO <= HI <= 100")
        return self


def parse_sigma_list(text: str, who: str, flag: str, counts: Sequence[int]):
    """'A,B,...' -> floats; SystemExit naming the flag when a field is no number or the count is not one of `counts`."""
    try:
        vals = [float(t) for t in str(text).split(",")]
    except ValueError:
        raise SystemExit(f"{who}: {flag} {text!r}: comma-separated numbers expected")
    if len(vals) not in counts:
        raise SystemExit(f"{who}: {flag} {text!r}: {' or '.join(str(c) for c in counts)} value(s) expected")
    return vals
