"""CPU: pesr_amd/csrc/resize_to.hip compiled as plain C++ into a stand-alone program (tests/host_build.py:
the lanes of a workgroup as threads, __syncthreads as a barrier) and run on the host - both passes,
the descriptor checks and the grid walk as they are - against the float64 restatement tests/resize_to_oracle.py, bit for bit.
Nothing is loaded into Python; no GPU is involved."""
import numpy as np
import pytest

import host_build
import resize_to_oracle as RT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_build.build("resize_to", tmp_path_factory.mktemp("resize_to_host"))


def _bits(x):
    from pesr_amd._pool import f64_bits
    return f64_bits(x)


class Tables:
    """The table buffer of a call, tap-major per table as include/pesr_hip.h lays it out."""

    def __init__(self):
        self.words, self.at = [], {}

    def get(self, n_in, n_out, m):
        from pesr_amd.resize import resize_table
        if (n_in, n_out, m) not in self.at:
            first, w = resize_table(n_in, n_out, m)
            self.at[(n_in, n_out, m)] = (sum(a.size for a in self.words), w.shape[1])
            self.words += [first.astype(np.int64), np.ascontiguousarray(w.T).reshape(-1).view(np.int64)]
        return self.at[(n_in, n_out, m)]

    def buffer(self):
        return np.concatenate(self.words)


def _run(program, axis, pool, rows, table, dst_bytes, n=None):
    head = np.array([len(rows) if n is None else n, axis, pool.size, table.size, dst_bytes], dtype=np.int64)
    return host_build.run(program, [head.tobytes(), np.array(rows, dtype=np.int64).tobytes(), table.tobytes(), pool.tobytes()])


def _mid(img, ho, m):
    return RT._round(RT.resize_axis0(img.astype(np.float64), ho, m))


CASES = (((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 7), (1, 1)), ((9, 13), (4, 29)), ((3, 345), (2, 100)), ((2, 100), (3, 345)), ((16, 16), (2, 2)),
         ((2, 2), (16, 16)))


@pytest.mark.parametrize("method", RT.METHODS)
def test_both_passes_on_the_host_equal_the_restatement(program, method):
    rng = np.random.default_rng(5)
    for (h, w), (ho, wo) in CASES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        tb = Tables()
        at0, T0 = tb.get(h, ho, method)
        at1, T1 = tb.get(w, wo, method)
        rc, mid = _run(program, 0, img.reshape(-1), [(0, w, 0, w, h, w, ho, w, at0, T0, 0, 0)], tb.buffer(), 3 * ho * w)
        assert rc == 0 and np.array_equal(mid.reshape(ho, w, 3), _mid(img, ho, method)), ((h, w), (ho, wo), "height")
        rc, out = _run(program, 1, mid, [(0, w, 0, wo, ho, w, ho, wo, at1, T1, 0, 0)], tb.buffer(), 3 * ho * wo)
        assert rc == 0 and np.array_equal(out.reshape(ho, wo, 3), RT.resize(img, (ho, wo), method)), ((h, w), (ho, wo), "width")


def test_strided_windows_at_odd_offsets_and_noise(program):
    """Three windows of one 24 x 40 image that starts 5 bytes into the pool, a filter and an output size each, written as windows of a
    20 x 50 destination image that starts 7 bytes into its buffer; the width pass adds noise to two of them."""
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    flat = np.concatenate([np.full(5, 77, np.uint8), img.reshape(-1)])
    wins = [(0, 0, 15, 17, (7, 17), (7, 30), "bicubic", 0.0, 0), (0, 17, 24, 23, (9, 23), (9, 5), "bilinear", 6.5, 12345),
            (16, 1, 8, 9, (11, 9), (11, 13), "box", 2.25, (1 << 64) - 3)]
    tb, rows0, rows1, places = Tables(), [], [], [(0, 0), (8, 20), (9, 1)]
    for (y0, x0, h, w, (hm, wm), (ho, wo), m, sig, q), (dy, dx) in zip(wins, places):
        at0, T0 = tb.get(h, hm, m)
        at1, T1 = tb.get(w, wo, m)
        rows0.append((5 + 3 * (y0 * 40 + x0), 40, 7 + 3 * (dy * 50 + dx), 50, h, w, hm, w, at0, T0, 0, 0))
        rows1.append((7 + 3 * (dy * 50 + dx), 50, 7 + 3 * (dy * 50 + dx), 50, hm, w, ho, wo, at1, T1, _bits(sig), q - (1 << 64) if q >> 63 else q))
    nbytes = 7 + 3 * 20 * 50
    rc, mid = _run(program, 0, flat, rows0, tb.buffer(), nbytes)
    assert rc == 0
    want = np.full(nbytes, 9, np.uint8)
    canvas = want[7:].reshape(20, 50, 3)
    for (y0, x0, h, w, (hm, wm), _, m, _, _), (dy, dx) in zip(wins, places):
        canvas[dy:dy + hm, dx:dx + w] = _mid(img[y0:y0 + h, x0:x0 + w], hm, m)
    assert np.array_equal(mid, want)                                       # every window right, and not a byte outside them touched
    # width pass from those windows into a fresh buffer (main.cpp's destination is not its source)
    rc, out = _run(program, 1, mid, rows1, tb.buffer(), nbytes)
    assert rc == 0
    want = np.full(nbytes, 9, np.uint8)
    canvas = want[7:].reshape(20, 50, 3)
    for (y0, x0, h, w, _, (ho, wo), m, sig, q), (dy, dx) in zip(wins, places):
        canvas[dy:dy + ho, dx:dx + wo] = RT.resize(img[y0:y0 + h, x0:x0 + w], (ho, wo), m, sig, q)
    assert np.array_equal(out, want)


def test_refused_descriptors_launch_nothing(program):
    tb = Tables()
    at, T = tb.get(8, 4, "bicubic")
    table = tb.buffer()
    pool = np.zeros(3 * 8 * 8, np.uint8)
    good0 = (0, 8, 0, 8, 8, 8, 4, 8, at, T, 0, 0)
    good1 = (0, 8, 0, 4, 8, 8, 8, 4, at, T, _bits(1.5), 7)
    assert _run(program, 0, pool, [good0], table, 96)[0] == 0 and _run(program, 1, pool, [good1], table, 96)[0] == 0

    def bad(row, i, v):
        return row[:i] + (v,) + row[i + 1:]
    cases = [(0, bad(good0, 0, -1)), (0, bad(good0, 2, -3)), (0, bad(good0, 1, 7)), (0, bad(good0, 3, 7)), (0, bad(good0, 4, 0)),
             (0, bad(good0, 6, 0)), (0, bad(good0, 5, 0)), (0, bad(good0, 9, 0)), (0, bad(good0, 9, 33)), (0, bad(good0, 8, -1)),
             (0, bad(good0, 8, table.size - T * 4)), (0, bad(good0, 10, _bits(1.0))), (0, bad(good0, 7, 4)),
             (0, bad(bad(good0, 4, 33), 6, 4)), (0, bad(bad(good0, 4, 1), 6, 9)),
             (1, bad(good1, 10, _bits(-1.0))), (1, bad(good1, 10, _bits(float("nan")))), (1, bad(good1, 10, _bits(float("inf")))),
             (1, bad(good1, 6, 4)), (1, bad(bad(good1, 5, 33), 7, 4)), (2, good0), (-1, good0)]
    for axis, row in cases:
        rc, out = _run(program, axis, pool, [row], table, 96)
        assert rc == 255 and (out == 9).all(), (axis, row)                  # (PESR_EINVAL = -1 as an exit status)
    rc, out = _run(program, 0, pool, [good0], table, 96, n=0)
    assert rc == 255 and (out == 9).all()


def test_the_products_plan_drives_both_passes_to_the_restatement(program):
    """pesr_amd.resize.resize_to_plan - the host half of imresize_to_pool_u8: tables, descriptors, offsets - fed to the host-compiled
    kernels as the library would get it: four entries of one call, a filter each, two sharing a table, noise on two, and the jitter's
    round trip 6 x 6 -> 1 x 1 -> 6 x 6 at the 8:1 clamp."""
    from pesr_amd.resize import resize_to_plan
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((9, 13), (9, 13), (6, 6), (5, 16))]
    outs, methods = [(4, 29), (4, 20), (1, 1), (40, 2)], ["bicubic", "bicubic", "box", "bilinear"]
    sigma, q = [0.0, 3.5, 0.0, 12.0], [0, 77, 0, (1 << 64) - 1]
    pool = np.concatenate([np.full(3, 1, np.uint8)] + [im.reshape(-1) for im in imgs])
    offs = [int(v) for v in 3 + np.cumsum([0] + [im.size for im in imgs[:-1]])]
    buf, (d0, d1), mid_bytes, out_off, shapes = resize_to_plan(offs, [im.shape[:2] for im in imgs], outs, methods, [im.shape[1] for im in imgs],
                                                               sigma, q)
    assert shapes == outs and d0.shape == d1.shape == (4, 12) and d0[0, 8] == d0[1, 8] and d1[0, 8] != d1[1, 8]      # 9 -> 4 shared, 13 -> 29 / 20 not
    rc, mid = _run(program, 0, pool, d0, buf, mid_bytes)
    assert rc == 0
    rc, out = _run(program, 1, mid, d1, buf, int(out_off[-1]))
    assert rc == 0
    for i, im in enumerate(imgs):
        ho, wo = outs[i]
        assert np.array_equal(out[out_off[i]:out_off[i + 1]].reshape(ho, wo, 3), RT.resize(im, (ho, wo), methods[i], sigma[i], q[i])), i
    back = resize_to_plan([0], [(1, 1)], [(6, 6)], ["bilinear"], [1], [2.0], [5])
    rc, mid = _run(program, 0, out[out_off[2]:out_off[3]], back[1][0], back[0], back[2])
    rc2, res = _run(program, 1, mid, back[1][1], back[0], 108)
    assert rc == 0 and rc2 == 0 and np.array_equal(res.reshape(6, 6, 3), RT.jitter(imgs[2], 0.125, 2, 1, 2.0, 5))
