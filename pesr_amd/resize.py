"""Bicubic resize of uint8 HWC images by an integer factor s in {2, 3, 4}, down (antialiased) and up, on the device: MATLAB's
imresize for uint8 input as pinned in docs/modes.md section 4f (Keys kernel a = -0.5, symmetric reflection at the border, float64
accumulation in ascending tap order without fused multiply-add, round half up, height pass then width pass with a uint8
intermediate).  Kernels: csrc/resize.hip.  The weights are made here, on the host, in float64 and cross the C ABI by value.
"""
from __future__ import annotations

import ctypes
import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _pool

SCALES = (2, 3, 4)
METHODS = ("bicubic", "bilinear", "box")           # the filters of the any-size resize (docs/modes.md section 4m)
MAX_RATIO = 8                                      # n_in <= 8 n_out and n_out <= 8 n_in on each axis
MAX_TAPS = 32
TO_DESC_WORDS = 12                                 # int64 words per descriptor row of pesr_resize_to_u8_pass (include/pesr_hip.h)


def _keys(num: int, den: int) -> float:
    """k(num / den): the argument is one integer divided once; products and sums left to right."""
    x = abs(num) / den
    x2 = x * x
    x3 = x2 * x
    if x <= 1.0:
        return 1.5 * x3 - 2.5 * x2 + 1.0
    if x <= 2.0:
        return -0.5 * x3 + 2.5 * x2 - 4.0 * x + 2.0
    return 0.0


def down_offsets(s: int) -> List[int]:
    """Tap offsets t of the down-resize (input index s*o + t): all integers with |2t - (s-1)| < 4s."""
    return [t for t in range(-2 * s - 1, 3 * s) if abs(2 * t - (s - 1)) < 4 * s]


def up_first_tap(s: int, p: int) -> int:
    """Phase p of the up-resize (output s*q + p) reads inputs q + d ... q + d + 3; -> d."""
    return -2 if 2 * p + 1 - s < 0 else -1


def resize_weights(s: int, up: bool) -> np.ndarray:
    """float64 weights, normalised by their sum in ascending tap order: shape [taps] (down: 8 / 11 / 16 at x2 / x3 / x4, the two
    zeros at x3 kept) or [s][4] (up, one row per output phase).  Host only."""
    if s not in SCALES:
        raise ValueError(f"resize factor {s} is not supported (2, 3, 4)")
    rows = []
    if up:
        for p in range(s):
            d = up_first_tap(s, p)
            rows.append([_keys(2 * s * (d + i) - (2 * p + 1 - s), 2 * s) for i in range(4)])
    else:
        rows.append([_keys(2 * t - (s - 1), 2 * s) for t in down_offsets(s)])
    out = []
    for raw in rows:
        total = 0.0
        for v in raw:
            total = total + v
        out.append([v / total for v in raw])
    w = np.array(out, dtype=np.float64)
    return w if up else w[0]


def modcrop(img: np.ndarray, s: int) -> np.ndarray:
    """Crop at the top-left to sides that are multiples of s."""
    h, w = img.shape[0], img.shape[1]
    return img[:h - h % s, :w - w % s]


def _out_len(n: int, s: int, up: bool) -> int:
    return n * s if up else n // s


def imresize_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], s: int, up: bool = False):
    """Resize every image of a flat device-resident uint8 pool (image i: HWC bytes at offsets[i], shapes[i] = (H, W)) in two
    launches.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    _pool.check_pool(pool, "imresize_pool_u8")
    n = len(offsets)
    assert n == len(shapes) and n > 0
    if s not in SCALES:
        raise _lib.PesrHipError(f"imresize: factor {s} is not supported (2, 3, 4)")
    for off, (h, w) in zip(offsets, shapes):
        assert 0 <= off and off + 3 * h * w <= pool.numel(), "image outside the pool"
        # (the library checks each pass's own axis again; checked here for both so that a bad width stops the height pass too)
        if h < 1 or w < 1 or (not up and (h % s or w % s)):
            raise _lib.PesrHipError(f"imresize: a {h} x {w} image cannot be reduced by {s}: mod-crop it first (modcrop)")
    mid_shapes = [(_out_len(h, s, up), w) for h, w in shapes]
    out_shapes = [(h, _out_len(w, s, up)) for h, w in mid_shapes]
    mid_off = np.concatenate([[0], np.cumsum([3 * h * w for h, w in mid_shapes])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([3 * h * w for h, w in out_shapes])]).astype(np.int64)
    dev = pool.device
    wts = np.zeros(16, dtype=np.float64)
    w = resize_weights(s, up).reshape(-1)
    wts[:w.size] = w
    mid = torch.empty(max(int(mid_off[-1]), 1), dtype=torch.uint8, device=dev)
    out = torch.empty(max(int(out_off[-1]), 1), dtype=torch.uint8, device=dev)
    wp = wts.ctypes.data_as(ctypes.c_void_p)
    passes = ((pool, mid, offsets, mid_off, shapes, 0), (mid, out, mid_off, out_off, mid_shapes, 1))
    for src, dst, so, do, shp, axis in passes:
        desc = np.array([(int(so[i]), int(do[i]), shp[i][0], shp[i][1]) for i in range(n)], dtype=np.int64)
        _pool.launch("pesr_imresize_u8_pass", src, dst, desc, axis, int(s), int(bool(up)), wp)
    return out[:int(out_off[-1])], [int(v) for v in out_off[:-1]], out_shapes


def imresize_u8(img: torch.Tensor, s: int, up: bool = False) -> torch.Tensor:
    """uint8 HWC device tensor -> uint8 HWC device tensor, sides divided (up=False; they must be multiples of s) or multiplied by s."""
    flat, h, w = _pool.image_as_pool(img, "imresize_u8")
    out, _, [(ho, wo)] = imresize_pool_u8(flat, [0], [(h, w)], s, up)
    return out.view(ho, wo, 3)


# ---- from any size to any size, three filters (docs/modes.md section 4m; kernels: csrc/resize_to.hip) --------------------------------

def _check_axis(n_in: int, n_out: int, method: str):
    if method not in METHODS:
        raise ValueError(f"resize filter {method!r} is not one of {', '.join(METHODS)}")
    if n_in < 1 or n_out < 1 or n_in > MAX_RATIO * n_out or n_out > MAX_RATIO * n_in:
        raise ValueError(f"resize of {n_in} to {n_out}: lengths >= 1 within {MAX_RATIO}:1 of each other expected")


@functools.lru_cache(maxsize=1024)
def _table(n_in: int, n_out: int, method: str):
    _check_axis(n_in, n_out, method)
    M = max(n_in, n_out)
    c = (2 * np.arange(n_out, dtype=np.int64) + 1) * n_in
    # taps: every j with lo <= N <= hi, N = (2j+1) n_out - (2o+1) n_in
    half = {"bicubic": 4 * M, "bilinear": 2 * M, "box": M}[method]
    lo, hi = (-M if method == "box" else 1 - half), half - 1
    first = (-((-(c + lo)) // n_out)) // 2                      # smallest j with 2j + 1 >= ceil((c + lo) / n_out)
    last = ((c + hi) // n_out - 1) // 2                         # largest j with 2j + 1 <= floor((c + hi) / n_out)
    T = int((last - first).max()) + 1
    j = first[:, None] + np.arange(T, dtype=np.int64)[None, :]
    N = (2 * j + 1) * n_out - c[:, None]
    x = np.abs(N) / (2 * M)                                     # one integer divided once
    if method == "bicubic":                                     # _keys, elementwise: the same products and sums, left to right
        x2 = x * x
        x3 = x2 * x
        raw = np.where(x <= 1.0, 1.5 * x3 - 2.5 * x2 + 1.0, np.where(x <= 2.0, -0.5 * x3 + 2.5 * x2 - 4.0 * x + 2.0, 0.0))
    elif method == "bilinear":
        raw = np.where(x <= 1.0, 1.0 - x, 0.0)
    else:
        raw = np.ones_like(x)
    raw = np.where(j <= last[:, None], raw, 0.0)                # rows with fewer taps end in 0.0
    total = np.cumsum(raw, axis=1)[:, -1]                       # (cumsum adds strictly left to right; the padding adds nothing)
    w = raw / total[:, None]
    first.setflags(write=False)
    w.setflags(write=False)
    return first, w


def resize_table(n_in: int, n_out: int, method: str = "bicubic"):
    """-> (first[n_out] int64, weights[n_out][T] float64): output o is the sum over k = 0 .. T-1 of weights[o][k] * in[reflect(first[o]
    + k)], with N = (2j+1) n_out - (2o+1) n_in, M = max(n_in, n_out), kernel argument N / (2M), taps all j with |N| < 4M (bicubic),
    |N| < 2M (bilinear), -M <= N < M (box); each row divided by its sum taken in ascending order, rows with fewer than T taps ending
    in 0.0.  Host only."""
    first, w = _table(int(n_in), int(n_out), str(method))
    return first.copy(), w.copy()


def resize_to_plan(offsets, shapes, out_shapes, methods, strides, noise_sigma, noise_stream):
    """Host half of imresize_to_pool_u8: -> (table buffer int64 [words], (height-pass descriptors, width-pass descriptors) int64
    [n][12], bytes of the intermediate pool, output byte offsets [n + 1], output shapes).  One table per distinct (n_in, n_out, method),
    shared by the entries and passes that use it; intermediate and output images lie back to back."""
    n = len(offsets)
    tables, words = {}, 0                                       # (n_in, n_out, method) -> (word offset, T, first, weights)
    for (h, w), (ho, wo), m in zip(shapes, out_shapes, methods):
        for n_in, n_out in ((h, ho), (w, wo)):
            try:
                _check_axis(n_in, n_out, m)
            except ValueError as e:
                raise _lib.PesrHipError(f"imresize_to: {e}")
            if (n_in, n_out, m) not in tables:
                first, wt = _table(n_in, n_out, m)
                tables[(n_in, n_out, m)] = (words, wt.shape[1], first, wt)
                words += (wt.shape[1] + 1) * n_out
    buf = np.empty(words, dtype=np.int64)
    for (n_in, n_out, m), (at, T, first, wt) in tables.items():
        buf[at:at + n_out] = first
        buf[at + n_out:at + (T + 1) * n_out] = np.ascontiguousarray(wt.T).reshape(-1).view(np.int64)   # tap-major
    out_shapes = [(int(ho), int(wo)) for ho, wo in out_shapes]
    mid_off = np.concatenate([[0], np.cumsum([3 * ho * w for (h, w), (ho, wo) in zip(shapes, out_shapes)])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([3 * ho * wo for ho, wo in out_shapes])]).astype(np.int64)
    d0 = np.empty((n, TO_DESC_WORDS), dtype=np.int64)
    d1 = np.empty((n, TO_DESC_WORDS), dtype=np.int64)
    for i in range(n):
        (h, w), (ho, wo), m = shapes[i], out_shapes[i], methods[i]
        at, T = tables[(h, ho, m)][:2]
        d0[i] = (int(offsets[i]), int(strides[i]), int(mid_off[i]), w, h, w, ho, w, at, T, 0, 0)
        at, T = tables[(w, wo, m)][:2]
        d1[i] = (int(mid_off[i]), w, int(out_off[i]), wo, ho, w, ho, wo, at, T, _pool.f64_bits(noise_sigma[i]), _pool.i64(int(noise_stream[i])))
    return buf, (d0, d1), int(mid_off[-1]), out_off, out_shapes


def imresize_to_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], out_shapes: Sequence[Tuple[int, int]],
                        methods, strides: Optional[Sequence[int]] = None, noise_sigma: Optional[Sequence[float]] = None,
                        noise_stream: Optional[Sequence[int]] = None):
    """Resize windows of a flat device-resident uint8 pool (entry i: shapes[i] = (h, w) HWC pixels from byte offsets[i], rows
    strides[i] pixels apart, None = w) to out_shapes[i] with filter methods[i] (one name serves every entry) in two launches: height,
    then width.  noise_sigma[i] / noise_stream[i]: section 4j's noise, added before the last rounding.  The reflection is at the
    window's own border.  -> (out_pool, out_offsets, out_shapes), the results back to back."""
    _pool.check_pool(pool, "imresize_to_pool_u8")
    n = len(offsets)
    methods = [methods] * n if isinstance(methods, str) else list(methods)
    strides = [w for _, w in shapes] if strides is None else list(strides)
    noise_sigma = [0.0] * n if noise_sigma is None else list(noise_sigma)
    noise_stream = [0] * n if noise_stream is None else list(noise_stream)
    assert n > 0 and n == len(shapes) == len(out_shapes) == len(methods) == len(strides) == len(noise_sigma) == len(noise_stream)
    for (h, w), off, st in zip(shapes, offsets, strides):
        assert st >= w and 0 <= off and off + 3 * ((h - 1) * st + w) <= pool.numel(), "window outside the pool"
    buf, descs, mid_bytes, out_off, out_shapes = resize_to_plan(offsets, shapes, out_shapes, methods, strides, noise_sigma, noise_stream)
    dev = pool.device
    buf_dev = torch.from_numpy(buf).to(dev)
    mid = torch.empty(max(mid_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(max(int(out_off[-1]), 1), dtype=torch.uint8, device=dev)
    for axis, desc in enumerate(descs):
        src, dst = (pool, mid) if axis == 0 else (mid, out)
        _pool.launch("pesr_resize_to_u8_pass", src, dst, desc, axis, buf_dev.data_ptr(), int(buf.size))
    return out[:int(out_off[-1])], [int(v) for v in out_off[:-1]], out_shapes


def imresize_to_u8(img: torch.Tensor, size: Tuple[int, int], method: str = "bicubic") -> torch.Tensor:
    """uint8 HWC device tensor -> uint8 HWC device tensor of size = (h_out, w_out)."""
    flat, h, w = _pool.image_as_pool(img, "imresize_to_u8")
    out, _, [(ho, wo)] = imresize_to_pool_u8(flat, [0], [(h, w)], [(int(size[0]), int(size[1]))], method)
    return out.view(ho, wo, 3)
