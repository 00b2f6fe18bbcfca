"""Restatement of tiled inference (docs/modes.md section 4h) in plain torch slicing, with its OWN plan arithmetic - TEST
INFRASTRUCTURE.  Loop over tiles, slice, call the model (or test.py:x8_forward) on the slice, copy the owned part.  Pinned on the
CPU with helpers.x8_toy_model (tests/test_tile_cpu.py): with a halo of one pixel it equals the whole-image result bit for bit."""
import torch


def axis(n, core, halo):
    """-> (t, [(start, lo, hi)]) written as a walk along the axis, not as pesr_amd.tile's closed form."""
    t = core + 2 * halo
    if t > n:
        t = n
    out, lo = [], 0
    while lo < n:
        hi = lo + core if lo + core < n else n
        start = lo - halo
        if start < 0:
            start = 0
        if start + t > n:
            start = n - t
        out.append((start, lo, hi))
        lo = hi
    return t, out


def tiles(H, W, core, halo):
    th, rows = axis(H, core, halo)
    tw, cols = axis(W, core, halo)
    return th, tw, [(y0, x0, a, b, c - a, d - b) for (y0, a, c) in rows for (x0, b, d) in cols]


def tiled(img, fn, scale, core, halo):
    """img [1,3,H,W]; fn: [1,3,h,w] -> [1,3,s*h,s*w]."""
    H, W = img.shape[2], img.shape[3]
    th, tw, ts = tiles(H, W, core, halo)
    s = scale
    out = None
    for (y0, x0, oy, ox, oh, ow) in ts:
        y = fn(img[:, :, y0:y0 + th, x0:x0 + tw].contiguous())
        if out is None:
            out = torch.full((1, 3, s * H, s * W), float("nan"), dtype=y.dtype, device=y.device)
        out[:, :, s * oy:s * (oy + oh), s * ox:s * (ox + ow)] = y[:, :, s * (oy - y0):s * (oy - y0 + oh), s * (ox - x0):s * (ox - x0 + ow)]
    return out


def member(t, m):
    """Entry m of test.py:x8_forward's inputs, t [..., h, w]."""
    if m & 1:
        t = t.flip(-1)
    if m & 2:
        t = t.flip(-2)
    if m & 4:
        t = t.transpose(-1, -2)
    return t.contiguous()


def unmember(o, m):
    if m & 4:
        o = o.transpose(-1, -2)
    if m & 2:
        o = o.flip(-2)
    if m & 1:
        o = o.flip(-1)
    return o


def gather(chw, desc, oh, ow):
    """chw [3,H,W] float; desc rows (y0, x0, m) -> [n,3,oh,ow]."""
    out = []
    for (y0, x0, m) in desc:
        th, tw = (ow, oh) if m & 4 else (oh, ow)
        out.append(member(chw[:, y0:y0 + th, x0:x0 + tw], m))
    return torch.stack(out)


def scatter(entries, desc, E, th, tw, s, H, W, p=None, wa=None, wb=None, out=None):
    """entries: list (per tile) of lists of E tensors [3, ., .] -> fp32 [3, sH, sW] by the expressions of csrc/tile.hip, each a
    separate torch op (nothing fused)."""
    if out is None:
        out = torch.full((3, s * H, s * W), float("nan"), dtype=torch.float32, device=entries[0][0].device)
    for k, (y0, x0, oy, ox, oh, ow) in enumerate(desc):
        v = unmember(entries[k][0], 0)
        for m in range(1, E):
            v = v + unmember(entries[k][m], m)
        if E == 8:
            v = v / 8
        if p is not None:
            v = torch.tensor(wa, dtype=torch.float32, device=v.device) * p[k] + torch.tensor(wb, dtype=torch.float32, device=v.device) * v
        out[:, s * oy:s * (oy + oh), s * ox:s * (ox + ow)] = v[:, s * (oy - y0):s * (oy - y0 + oh), s * (ox - x0):s * (ox - x0 + ow)]
    return out


def to_u8(f):
    """[3, h, w] float -> uint8 [h, w, 3]: clamp to 0..255, round half to even."""
    return f.clamp(0, 255).round().permute(1, 2, 0).contiguous().to(torch.uint8)
