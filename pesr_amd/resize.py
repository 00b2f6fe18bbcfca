"""Bicubic resize of uint8 HWC images by an integer factor s in {2, 3, 4}, down (antialiased) and up, on the device: MATLAB's
imresize for uint8 input as pinned in docs/modes.md section 4f (Keys kernel a = -0.5, symmetric reflection at the border, float64
accumulation in ascending tap order without fused multiply-add, round half up, height pass then width pass with a uint8
intermediate).  Kernels: csrc/resize.hip.  The weights are made here, on the host, in float64 and cross the C ABI by value.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SCALES = (2, 3, 4)


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
    if not (torch.is_tensor(pool) and pool.is_cuda):
        raise _lib.PesrHipError("imresize_pool_u8 needs a device tensor: pesr_amd has no CPU fallback")
    assert pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()
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
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    mid = torch.empty(max(int(mid_off[-1]), 1), dtype=torch.uint8, device=dev)
    out = torch.empty(max(int(out_off[-1]), 1), dtype=torch.uint8, device=dev)
    wp = wts.ctypes.data_as(ctypes.c_void_p)
    passes = ((pool, mid, offsets, mid_off, shapes, 0), (mid, out, mid_off, out_off, mid_shapes, 1))
    for src, dst, so, do, shp, axis in passes:
        desc = np.array([(int(so[i]), int(do[i]), shp[i][0], shp[i][1]) for i in range(n)], dtype=np.int64)
        desc_dev = torch.from_numpy(desc).to(dev)          # the library checks the host copy; the kernel reads this one
        _lib.check(L.pesr_imresize_u8_pass(src.data_ptr(), dst.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), desc_dev.data_ptr(), n, axis,
                                           int(s), int(bool(up)), wp, stream), "pesr_imresize_u8_pass")
    return out[:int(out_off[-1])], [int(v) for v in out_off[:-1]], out_shapes


def imresize_u8(img: torch.Tensor, s: int, up: bool = False) -> torch.Tensor:
    """uint8 HWC device tensor -> uint8 HWC device tensor, sides divided (up=False; they must be multiples of s) or multiplied by s."""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise _lib.PesrHipError("imresize_u8 needs a device tensor: pesr_amd has no CPU fallback")
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, "uint8 [H][W][3] expected"
    h, w = int(img.shape[0]), int(img.shape[1])
    out, _, [(ho, wo)] = imresize_pool_u8(img.contiguous().view(-1), [0], [(h, w)], s, up)
    return out.view(ho, wo, 3)
