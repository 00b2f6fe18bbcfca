"""CPU float64 restatement of the JPEG round trip of docs/modes.md section 4l, written from the definition and sharing no code with
pesr_amd/jpeg.py: what a baseline encoder at quality q followed by a decoder returns for a uint8 HWC RGB image, without the
(lossless) entropy coding.

Tables: Annex K scaled the IJG way.  Colour: JFIF full range, every product and sum rounded separately, 8-bit samples between the
stages (clamp, floor(v + 0.5)).  4:2:0: chroma planes of ceil(h/2) x ceil(w/2), the 2 x 2 mean rounded half up; back up with the
9/3/3/1 triangle filter, rounded half up.  Blocks anchored at the image origin, planes extended to multiples of 8 by replicating the
last row and column.  DCT: the orthonormal 8 x 8 DCT-II from a table of eight pinned float64 values, rows then columns, sums in
ascending order; k = sign(F) floor(|F| / Q + 0.5), F' = k Q; inverse columns then rows.  Vectorised over blocks, sequential over
the eight terms of every sum, as numpy rounds each product and each sum of float64 arrays separately.
"""
import numpy as np

# Annex K, tables K.1 and K.2, in natural (row = vertical frequency) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61,
                 12, 12, 14, 19, 26, 58, 60, 55,
                 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77,
                 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99,
                   18, 21, 26, 66, 99, 99, 99, 99,
                   24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99,
                   99, 99, 99, 99, 99, 99, 99, 99,
                   99, 99, 99, 99, 99, 99, 99, 99,
                   99, 99, 99, 99, 99, 99, 99, 99,
                   99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64).reshape(8, 8)

# 0.5 cos(m pi / 16), m = 0 .. 7, with entry 0 standing for 0.5 sqrt(0.5) (u = 0); the values ARE the definition
HALF_COS = (0.3535533905932738, 0.4903926402016152, 0.46193976625564337, 0.4157348061512726, 0.3535533905932738,
            0.27778511650980114, 0.19134171618254492, 0.09754516100806417)


def quant_tables(q):
    """-> (luma, chroma) int64 [8][8] at quality q, 1 .. 100."""
    assert 1 <= q <= 100
    S = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * S + 50) // 100, 1, 255) for base in (LUMA, CHROMA))


def dct_table():
    """T[u][x] = 0.5 c(u) cos((2x+1) u pi / 16) from the eight pinned values: the angle folded into the first octant by symmetry."""
    T = np.empty((8, 8), dtype=np.float64)
    for u in range(8):
        for x in range(8):
            m = ((2 * x + 1) * u) % 32
            if m > 16:
                m = 32 - m
            sign = 1.0
            if m > 8:
                m, sign = 16 - m, -1.0
            T[u, x] = sign * HALF_COS[m]          # (m == 8 never happens for u < 8; m == 0 only for u == 0)
    return T


def round8(v):
    return np.floor(np.clip(v, 0.0, 255.0) + 0.5)


def rgb_to_ycc(img, rounded=True):
    a = np.asarray(img).astype(np.float64)
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    Y = (0.299 * R + 0.587 * G) + 0.114 * B
    Cb = ((128.0 - 0.168736 * R) - 0.331264 * G) + 0.5 * B
    Cr = ((128.0 + 0.5 * R) - 0.418688 * G) - 0.081312 * B
    return tuple(round8(p) if rounded else p for p in (Y, Cb, Cr))


def down420(p, rounded=True):
    """h x w -> ceil(h/2) x ceil(w/2): the mean of the 2 x 2 block, an odd side replicating its last row / column."""
    h, w = p.shape
    r0, c0 = np.arange(0, h, 2), np.arange(0, w, 2)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    s = ((p[r0][:, c0] + p[r0][:, c1]) + p[r1][:, c0]) + p[r1][:, c1]
    v = s * 0.25
    return np.floor(v + 0.5) if rounded else v


def up420(c, h, w):
    """ceil(h/2) x ceil(w/2) -> h x w, the triangle filter: 9/16 on the nearest chroma sample, 3/16 on the next in y and in x, 1/16 on
    the diagonal one, neighbours replicated at the plane's border; rounded half up."""
    ch, cw = c.shape
    y, x = np.arange(h), np.arange(w)
    cy, cx = y // 2, x // 2
    ny = np.clip(np.where(y % 2 == 1, cy + 1, cy - 1), 0, ch - 1)
    nx = np.clip(np.where(x % 2 == 1, cx + 1, cx - 1), 0, cw - 1)
    v = ((9.0 * c[cy][:, cx] + 3.0 * c[cy][:, nx]) + 3.0 * c[ny][:, cx]) + c[ny][:, nx]     # integers: exact
    return np.floor(v / 16.0 + 0.5)


def _blocks(p):
    """h x w plane -> [nby][nbx][8][8] of the plane extended to multiples of 8 by replication."""
    h, w = p.shape
    H, W = -(-h // 8) * 8, -(-w // 8) * 8
    e = p[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)]
    return e.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def fdct(blocks):
    """[..., 8(y), 8(x)] -> F[..., v, u]: rows first, G[y][u] = sum_x T[u][x] p[y][x], then columns, F[v][u] = sum_y T[v][y] G[y][u]."""
    T = dct_table()
    G = np.zeros(blocks.shape)
    for x in range(8):
        G = G + T[None, :, x] * blocks[..., :, x, None]          # [.., y, u]
    F = np.zeros(blocks.shape)
    for y in range(8):
        F = F + T[:, y, None] * G[..., None, y, :]               # [.., v, u]
    return F


def idct(F):
    """F[..., v, u] -> p[..., y, x]: columns first, H[y][u] = sum_v T[v][y] F[v][u], then rows, p[y][x] = sum_u T[u][x] H[y][u]."""
    T = dct_table()
    Hm = np.zeros(F.shape)
    for v in range(8):
        Hm = Hm + T[v, :, None] * F[..., None, v, :]             # [.., y, u]
    p = np.zeros(F.shape)
    for u in range(8):
        p = p + T[u, None, :] * Hm[..., :, u, None]              # [.., y, x]
    return p


def quantise(F, Q):
    kq = np.floor(np.abs(F) / Q + 0.5) * Q
    return np.where(F < 0, -kq, kq)


def code_plane(p, Q, rounded=True):
    """One 8-bit plane through level shift, DCT, quantise / dequantise, inverse DCT, level shift: h x w -> h x w."""
    h, w = p.shape
    b = idct(quantise(fdct(_blocks(p) - 128.0), Q.astype(np.float64))) + 128.0
    out = b.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8)[:h, :w]
    return round8(out) if rounded else out


def jpeg(img, q, chroma420=True, rounded=True):
    """uint8 HWC RGB -> uint8 HWC RGB after the round trip at quality q.  rounded=False drops every intermediate 8-bit rounding
    (colour samples, the 4:2:0 mean, the decoded planes; the triangle filter and the result keep theirs): not the definition, a
    variant to measure what the roundings are worth."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] >= 1 and img.shape[1] >= 1
    h, w = img.shape[:2]
    QL, QC = quant_tables(q)
    Y, Cb, Cr = rgb_to_ycc(img, rounded)
    if chroma420:
        Cb, Cr = down420(Cb, rounded), down420(Cr, rounded)
    Y, Cb, Cr = code_plane(Y, QL, rounded), code_plane(Cb, QC, rounded), code_plane(Cr, QC, rounded)
    if chroma420:
        Cb, Cr = up420(Cb, h, w), up420(Cr, h, w)
    cb, cr = Cb - 128.0, Cr - 128.0
    R = Y + 1.402 * cr
    G = (Y - 0.344136 * cb) - 0.714136 * cr
    B = Y + 1.772 * cb
    return round8(np.stack([R, G, B], axis=2)).astype(np.uint8)


def jpeg_window(pool, offset, stride, h, w, q, chroma420=True):
    """The round trip of the h x w window at byte `offset` of a flat uint8 pool, rows `stride` pixels apart."""
    rows = [np.asarray(pool[offset + 3 * stride * y:offset + 3 * stride * y + 3 * w]) for y in range(h)]
    return jpeg(np.stack(rows).reshape(h, w, 3), q, chroma420)
