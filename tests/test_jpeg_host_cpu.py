"""CPU: pesr_amd/csrc/jpeg.hip compiled as plain C++ into a stand-alone program (tests/host_build.py: the lanes of a workgroup as
threads, __syncthreads as a barrier) and run on the host - both launches, the descriptor checks and the grid walk as they are - against
the float64 restatement tests/jpeg_oracle.py, bit for bit.  Nothing is loaded into Python; no GPU is involved."""
import numpy as np
import pytest

import host_build
import jpeg_oracle as JO


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_build.build("jpeg", tmp_path_factory.mktemp("jpeg_host"))


def _run(program, pool, rows, c420, inplace):
    from pesr_amd.jpeg import dct_table, quant_tables
    quant = np.stack([np.stack(quant_tables(q)).reshape(2, 64) for q in range(1, 101)]).astype(np.float64)
    head = np.array([len(rows), 420 if c420 else 444, pool.size, int(inplace)], dtype=np.int64)
    return host_build.run(program, [head.tobytes(), np.array(rows, dtype=np.int64).tobytes(), dct_table().tobytes(), quant.tobytes(),
                                    pool.tobytes()])


@pytest.mark.parametrize("c420", [True, False])
def test_kernels_on_the_host_equal_the_restatement(program, c420):
    from pesr_amd.jpeg import entry_bytes
    rng = np.random.default_rng(11)
    for (h, w), q in (((1, 1), 50), ((15, 17), 10), ((17, 33), 75), ((3, 40), 1), ((32, 16), 100)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rc, out = _run(program, img.reshape(-1), [(0, w, 0, w, h, w, q, 0)], c420, False)
        assert rc == 0 and np.array_equal(out.reshape(h, w, 3), JO.jpeg(img, q, c420)), (h, w, q)
    # three windows of one 24 x 40 image at an odd offset, a quality each: out of place, then in place
    img = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    flat = np.concatenate([np.full(5, 77, np.uint8), img.reshape(-1)])
    wins = [(0, 0, 15, 17, 30), (0, 17, 24, 23, 85), (16, 1, 8, 9, 49)]
    rows, want_pool, oo, wo = [], flat.copy(), 0, 0
    for y0, x0, h, w, q in wins:
        off = 5 + 3 * (y0 * 40 + x0)
        rows.append((off, 40, oo, w, h, w, q, wo))
        oo += 3 * h * w
        wo += entry_bytes(h, w, c420)
        want = JO.jpeg(img[y0:y0 + h, x0:x0 + w], q, c420)
        for y in range(h):
            want_pool[off + 120 * y:off + 120 * y + 3 * w] = want[y].reshape(-1)
    rc, out = _run(program, flat, rows, c420, False)
    assert rc == 0
    for (y0, x0, h, w, q), r in zip(wins, rows):
        assert np.array_equal(out[r[2]:r[2] + 3 * h * w].reshape(h, w, 3), JO.jpeg(img[y0:y0 + h, x0:x0 + w], q, c420)), (y0, x0)
    rc, out = _run(program, flat, [(r[0], 40, r[0], 40) + r[4:] for r in rows], c420, True)
    assert rc == 0 and np.array_equal(out, want_pool)
    # refused descriptors: nothing runs, the destination keeps the program's fill value 9
    for bad in ((0, 40, 0, 17, 15, 17, 0, 0), (0, 16, 0, 17, 15, 17, 50, 0), (0, 40, 0, 17, 0, 17, 50, 0), (0, 40, 0, 17, 15, 17, 50, 8)):
        rc, out = _run(program, flat, [bad], c420, False)
        assert rc == 255 and (out == 9).all(), bad                            # (PESR_EINVAL = -1 as an exit status)
