"""Tiled inference (docs/modes.md section 4h): a full LR image as batches of overlapping tiles of ONE fixed shape.

The plan is pure Python.  The driver runs [gather, Generator, scatter] per batch: csrc/tile.hip's two kernels cut the tiles (and, for
the x8 self-ensemble, their eight flips / transposes) out of the image and put each tile's owned interior - averaged over the
ensemble and blended with a second model's output when asked - into the result, so nothing image-sized is made in between.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from . import ops


def receptive_halo(num_blocks: int, scale: int) -> int:
    """The halo in LR pixels from which on a tiled forward equals the whole-image forward up to fp32 summation order: embed 1,
    2 per ResBlock, trunk tail 1, upsample.0 1, and one more LR pixel for the convs that run at 2x / 3x / 4x resolution."""
    if scale not in (2, 3, 4):
        raise ValueError(f"receptive_halo: scale {scale} is not supported (2, 3, 4)")
    return 2 * int(num_blocks) + 4


def axis_plan(n: int, core: int, halo: int) -> Tuple[int, List[Tuple[int, int, int]]]:
    """One axis of length n -> (tile length t, [(start, own_lo, own_hi)]): t = min(core + 2*halo, n); tile c owns
    [c*core, min((c+1)*core, n)) and starts at clamp(c*core - halo, 0, n - t) - shifted inward at the far border, never cut."""
    n, core, halo = int(n), int(core), int(halo)
    if n < 1 or core < 1 or halo < 0:
        raise ValueError(f"axis_plan: need n >= 1, core >= 1, halo >= 0, got {n}, {core}, {halo}")
    t = min(core + 2 * halo, n)
    out = []
    for c in range(-(-n // core)):
        lo = c * core
        out.append((min(max(lo - halo, 0), n - t), lo, min(lo + core, n)))
    return t, out


def plan(H: int, W: int, core: int, halo: int):
    """-> (t_h, t_w, rows {y0, x0, oy, ox, oh, ow}): every tile's origin and the rectangle it owns (origin, rows, columns), row-major
    over the grid of tiles.  The owned rectangles partition the image: what pesr_tile_scatter's contract (no overlap) rests on."""
    th, rows = axis_plan(H, core, halo)
    tw, cols = axis_plan(W, core, halo)
    return th, tw, [(y0, x0, ylo, xlo, yhi - ylo, xhi - xlo) for y0, ylo, yhi in rows for x0, xlo, xhi in cols]


def blend_weights(alpha: float) -> Tuple[float, float]:
    """(float32(alpha), float32(1 - alpha)) with the subtraction in double: what torch makes of the Python scalars in
    `alpha * out + (1 - alpha) * out_psnr`."""
    return float(np.float32(alpha)), float(np.float32(1.0 - float(alpha)))


def _image(img: torch.Tensor):
    """-> (kernel source, H, W): fp32 [3, H, W] (a leading batch axis of 1 is dropped) or uint8 [H, W, 3]."""
    if img.dtype == torch.uint8:
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"tiled_forward: a uint8 image is [H, W, 3], got {tuple(img.shape)}")
        return img, int(img.shape[0]), int(img.shape[1])
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    if img.dtype != torch.float32 or img.dim() != 3 or img.shape[0] != 3:
        raise ValueError(f"tiled_forward: a float image is [3, H, W] or [1, 3, H, W] float32, got {tuple(img.shape)}")
    return img, int(img.shape[1]), int(img.shape[2])


def tiled_forward(model: Callable, img: torch.Tensor, scale: int, core: int, halo: int, batch: int = 16, ensemble: bool = False,
                  blend_model: Optional[Callable] = None, alpha: float = 1.0, f32: bool = True, u8: bool = False):
    """`model` (any callable [n, 3, h, w] -> [n, 3, s*h, s*w]) over the tiles of `img` -> (fp32 [1, 3, s*H, s*W] or None,
    uint8 [s*H, s*W, 3] or None).

    ensemble: every tile is run under the eight transforms of test.py:x8_forward and averaged.  blend_model: the result is
    alpha * blend_model(tile) + (1 - alpha) * that, test.py's `alpha * perceptual + (1 - alpha) * x8(psnr)`, formed inside the scatter.
    Every model call of an image with more tiles than a batch has the same shape: the last batch is filled up with repeats of a real
    tile whose outputs are dropped; an image with fewer tiles runs at its own count.  With `ensemble` a batch holds whole tiles
    (`batch` rounded down to a multiple of 8, at least 8); tiles that are not square run their members 0-3 and 4-7 as two calls."""
    if not (f32 or u8):
        raise ValueError("tiled_forward: nothing asked for (f32 and u8 both false)")
    if batch < 1:
        raise ValueError(f"tiled_forward: batch {batch}")
    src, H, W = _image(img)
    s = int(scale)
    th, tw, tiles = plan(H, W, core, halo)
    E = 8 if ensemble else 1
    per_call = max(int(batch) // 8, 1) if ensemble else int(batch)
    wa, wb = blend_weights(alpha) if blend_model is not None else (1.0, 0.0)
    dev = src.device
    out_f = torch.empty((3, s * H, s * W), dtype=torch.float32, device=dev) if f32 else None
    out_u = torch.empty((s * H, s * W, 3), dtype=torch.uint8, device=dev) if u8 else None
    with torch.no_grad():
        for first in range(0, len(tiles), per_call):
            real = tiles[first:first + per_call]
            run = real + [real[-1]] * (per_call - len(real) if len(tiles) > per_call else 0)
            if not ensemble:
                t_lo, t_hi = model(ops.tile_gather(src, [(t[0], t[1], 0) for t in run], th, tw)), None
            elif th == tw:
                t_lo, t_hi = model(ops.tile_gather(src, [(t[0], t[1], m) for t in run for m in range(8)], th, tw)), None
            else:
                t_lo = model(ops.tile_gather(src, [(t[0], t[1], m) for t in run for m in range(4)], th, tw))
                t_hi = model(ops.tile_gather(src, [(t[0], t[1], m) for t in run for m in range(4, 8)], tw, th))
            p = None
            if blend_model is not None:
                p = blend_model(ops.tile_gather(src, [(t[0], t[1], 0) for t in run], th, tw))[:len(real)]
            k = len(real) * (E if t_hi is None else 4)
            ops.tile_scatter(t_lo[:k], None if t_hi is None else t_hi[:k], real, E, th, tw, s, H, W, out_f, out_u, p, wa, wb)
    return (out_f[None] if f32 else None), out_u


def describe(core: int, halo: int, exact: int, attention: bool = False, wattn: bool = False) -> str:
    """The line the entry points print once per run: tile shape, halo, the exact halo, and whether the results are the whole-image
    forward or an approximation of it.  (Facts of the run only: the number of tiles differs from image to image.)  attention: the
    Generator pools every block's features over whatever it is given (docs/modes.md section 4u) - a tile's mean is not the image's,
    so no halo is exact.  wattn: the Generator has window-attention blocks (docs/modes.md section 4w), whose window grid starts at the
    tile's corner and not at the image's - one more sentence says so."""
    if wattn:
        return describe(core, halo, exact, attention) + \
            "; with the Generator's window-attention blocks an APPROXIMATION at every halo (their 8 x 8 window grid starts at the " \
            "tile, not at the image)"
    side = core + 2 * halo
    if attention:
        return f"Tiled: tiles of {side} x {side} (an image shorter than that on an axis is taken whole along it), core {core}, halo " \
               f"{halo}: an APPROXIMATION of the whole-image forward at every halo for every image larger than one tile (the " \
               f"Generator's channel attention pools over the tile, not over the image; its convs alone reach {exact} pixels)"
    line = f"Tiled: tiles of {side} x {side} (an image shorter than that on an axis is taken whole along it), core {core}, halo {halo}, " \
           f"exact halo {exact}"
    if halo < exact:
        line += ": an APPROXIMATION of the whole-image forward for every image larger than one tile (halo below the receptive field)"
    else:
        line += ": equals the whole-image forward up to fp32 summation order"
    return line


def check_flags(prog: str, names: Tuple[str, ...], core: int, halo: int, batch: int, num_blocks: int, scale: int) -> Optional[int]:
    """The entry points' flag checks: -> the halo to use (None when tiling is off); SystemExit naming the flag otherwise."""
    if core < 0:
        raise SystemExit(f"{prog}: {names[0]} is the side of a tile's owned square in LR pixels (0 = off), got {core}")
    if halo < -1:
        raise SystemExit(f"{prog}: {names[1]} is a width in LR pixels (or -1 for the exact halo, 2 * num_blocks + 4), got {halo}")
    if len(names) > 2 and batch < 1:
        raise SystemExit(f"{prog}: {names[2]} is the number of tiles per Generator call, at least 1, got {batch}")
    if core == 0:
        return None
    return receptive_halo(num_blocks, scale) if halo == -1 else halo
