"""The JPEG round trip on the device, as pinned in docs/modes.md section 4l: what a baseline encoder at quality q followed by a
decoder returns for a uint8 HWC RGB window - JFIF colour conversion, 4:2:0 or 4:4:4 chroma, 8 x 8 blocks anchored at the window's
origin, the Annex K tables scaled the IJG way, a float64 DCT - without the (lossless) entropy coding.  Kernel: csrc/jpeg.hip.  The
quantisation tables and the DCT table are made here, on the host; the device never evaluates cos.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _pool

DESC_WORDS = 8             # int64 words per descriptor row (include/pesr_hip.h)

# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major: row = vertical frequency
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# 0.5 cos(m pi / 16) for m = 1 .. 7; entry 0 is 0.5 sqrt(0.5), the u = 0 row.  These eight float64 values are the definition.
_HALF_COS = (0.3535533905932738, 0.4903926402016152, 0.46193976625564337, 0.4157348061512726, 0.3535533905932738, 0.27778511650980114,
             0.19134171618254492, 0.09754516100806417)


def quant_tables(q: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (luminance, chrominance), int64 [8][8]: clamp((base * S + 50) / 100, 1, 255) in integers, S = 5000 / q below 50 and
    200 - 2 q from 50 on (the IJG quality scale)."""
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg: quality {q} is outside 1 .. 100")
    S = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, dtype=np.int64).reshape(8, 8) * S + 50) // 100, 1, 255) for base in (_K1, _K2))


def dct_table() -> np.ndarray:
    """float64 [8][8]: T[u][x] = 0.5 c(u) cos((2x+1) u pi / 16), c(0) = sqrt(0.5), c(u) = 1 otherwise - every entry is plus or minus one
    of the eight pinned values, the angle reduced by the cosine's symmetries."""
    T = np.empty((8, 8), dtype=np.float64)
    for u in range(8):
        for x in range(8):
            m = (2 * x + 1) * u % 32
            m = 32 - m if m > 16 else m
            T[u, x] = -_HALF_COS[16 - m] if m > 8 else _HALF_COS[m]
    return T


_tables = {}


def _device_tables(dev: torch.device):
    """(T, the tables of q = 1 .. 100) on `dev`, uploaded once per device."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _tables:
        quant = np.stack([np.stack(quant_tables(q)).reshape(2, 64) for q in range(1, 101)]).astype(np.float64)
        _tables[key] = (torch.from_numpy(dct_table()).to(dev), torch.from_numpy(quant).to(dev))
    return _tables[key]


def entry_bytes(h: int, w: int, chroma420: bool) -> int:
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2) if chroma420 else 3 * h * w


def jpeg_pool_u8(pool: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], strides: Sequence[int], qualities: Sequence[int],
                 chroma420: bool = True, out: Optional[torch.Tensor] = None):
    """The round trip of n windows of a flat device-resident uint8 pool in ONE call: window i is shapes[i] = (h, w) pixels at byte
    offsets[i], its rows strides[i] pixels apart, compressed at qualities[i]; the block grid starts at the window's origin.  The
    windows must not overlap.  out = None: -> (out_pool, out_offsets), the results back to back, rows w pixels apart.  out = a
    tensor of the pool's size (the pool itself: in place): every result is written where its window lies in the pool, the bytes
    outside the windows are not touched, -> (out, offsets)."""
    _pool.check_pool(pool, "jpeg_pool_u8")
    n = len(offsets)
    assert n > 0 and n == len(shapes) == len(strides) == len(qualities)
    dev = pool.device
    if out is not None:
        assert torch.is_tensor(out) and out.device == dev and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()
        assert out.numel() == pool.numel(), "out: a tensor of the pool's size expected"
    desc = np.empty((n, DESC_WORDS), dtype=np.int64)
    out_off = ws_off = 0
    for i in range(n):
        (h, w), off, stride, q = shapes[i], int(offsets[i]), int(strides[i]), int(qualities[i])
        if h < 1 or w < 1 or stride < w:
            raise _lib.PesrHipError(f"jpeg: a {h} x {w} window with rows {stride} pixels apart is not legal")
        if not 1 <= q <= 100:
            raise _lib.PesrHipError(f"jpeg: quality {q} is outside 1 .. 100")
        assert 0 <= off and off + 3 * (stride * (h - 1) + w) <= pool.numel(), "window outside the pool"
        desc[i] = (off, stride, off, stride, h, w, q, ws_off) if out is not None else (off, stride, out_off, w, h, w, q, ws_off)
        out_off += 3 * h * w
        ws_off += entry_bytes(h, w, chroma420)
    if out is None:
        out = torch.empty(out_off, dtype=torch.uint8, device=dev)
    chroma = 420 if chroma420 else 444
    need = int(_lib.lib().pesr_jpeg_workspace_bytes(desc.ctypes.data_as(ctypes.c_void_p), n, chroma))
    assert need == ws_off, (need, ws_off)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    T, quant = _device_tables(dev)
    _pool.launch("pesr_jpeg_u8", pool, out, desc, chroma, T.data_ptr(), quant.data_ptr(), ws.data_ptr(), need)
    return out, [int(v) for v in desc[:, 2]]


def jpeg_u8(img: torch.Tensor, q: int, chroma420: bool = True) -> torch.Tensor:
    """uint8 HWC device tensor -> the uint8 HWC image a JPEG encoder at quality q and a decoder make of it."""
    flat, h, w = _pool.image_as_pool(img, "jpeg_u8")
    out, _ = jpeg_pool_u8(flat, [0], [(h, w)], [w], [q], chroma420)
    return out.view(h, w, 3)


def parse_quality(text: str, who: str, flag: str, count: int):
    """'Q' or 'LO,HI' -> ints in 1 .. 100 (LO <= HI); SystemExit naming the flag otherwise."""
    try:
        vals = [int(t) for t in str(text).split(",")]
    except ValueError:
        raise SystemExit(f"{who}: {flag} {text!r}: {'LO,HI' if count == 2 else 'one integer'} in 1 .. 100 expected")
    if len(vals) != count or not all(1 <= v <= 100 for v in vals) or vals != sorted(vals):
        raise SystemExit(f"{who}: {flag} {text!r}: {'LO,HI with 1 <= LO <= HI <= 100' if count == 2 else 'one integer in 1 .. 100'} expected")
    return vals
