"""What the byte-image front ends (resize.py, degrade.py, jpeg.py) share: the argument checks of a flat uint8 pool and of one HWC
image, the two integer encodings a descriptor word may need, and the step that hands a descriptor array to the library.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import torch

from . import _lib

_MASK = (1 << 64) - 1


def need_device(t, who: str):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.PesrHipError(f"{who} needs a device tensor: pesr_amd has no CPU fallback")


def check_pool(pool, who: str):
    """A flat, contiguous uint8 device tensor."""
    need_device(pool, who)
    assert pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()


def image_as_pool(img, who: str):
    """uint8 [H][W][3] device tensor -> (its bytes as a pool of one image, H, W)."""
    need_device(img, who)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, "uint8 [H][W][3] expected"
    return img.contiguous().view(-1), int(img.shape[0]), int(img.shape[1])


def f64_bits(x: float) -> int:
    """The bits of a float64 as the int64 a descriptor word holds."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def i64(q: int) -> int:
    """A 64-bit pattern (any Python int, taken mod 2**64) as an int64."""
    q &= _MASK
    return q - (1 << 64) if q >> 63 else q


def launch(entry: str, src: torch.Tensor, dst: torch.Tensor, desc: np.ndarray, *args):
    """Call the library's `entry`(src, dst, desc_host, desc_dev, n, *args, stream) for the n rows of the int64 array `desc` on src's
    device and current stream.  The library checks the host copy of the descriptors; the kernel reads the device copy made here."""
    desc_dev = torch.from_numpy(desc).to(src.device)
    stream = torch.cuda.current_stream(src.device).cuda_stream
    _lib.check(getattr(_lib.lib(), entry)(src.data_ptr(), dst.data_ptr(), desc.ctypes.data_as(ctypes.c_void_p), desc_dev.data_ptr(), len(desc),
                                          *args, stream), entry)
