"""CPU: pesr_amd/csrc/resize.hip compiled as plain C++ into a stand-alone program (tests/host_build.py: the lanes of a workgroup as
threads, __syncthreads as a barrier) and run on the host - both passes, the descriptor checks and the grid walk as they are - against
the float64 restatement tests/resize_oracle.py, bit for bit.  Nothing is loaded into Python; no GPU is involved."""
import numpy as np
import pytest

import host_build
import resize_oracle as RO


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_build.build("resize", tmp_path_factory.mktemp("resize_host"))


def _weights(s, up):
    from pesr_amd.resize import resize_weights
    wts = np.zeros(16, dtype=np.float64)
    w = resize_weights(s, up).reshape(-1)
    wts[:w.size] = w
    return wts


def _run(program, rows, axis, s, up, pool, dst_bytes, wts=None, n=None):
    head = np.array([len(rows) if n is None else n, axis, s, int(up), pool.size, dst_bytes], dtype=np.int64)
    wts = _weights(s, up) if wts is None else wts
    return host_build.run(program, [head.tobytes(), np.array(rows, dtype=np.int64).tobytes(), wts.tobytes(), pool.tobytes()])


def _mid(img, s, up):
    return RO.resize_axis0(img.astype(np.float64), s, up).astype(np.uint8)


def _olen(n, s, up):
    return n * s if up else n // s


def _odd(at):
    """The first offset past `at` that is no multiple of 4."""
    return at + (2 if (at + 1) % 4 == 0 else 1)


def _both_passes(program, img, s, up):
    h, w = img.shape[:2]
    ho, wo = _olen(h, s, up), _olen(w, s, up)
    rc, mid = _run(program, [(0, 0, h, w)], 0, s, up, img.reshape(-1), 3 * ho * w)
    assert rc == 0 and np.array_equal(mid.reshape(ho, w, 3), _mid(img, s, up)), (img.shape, s, up, "height")
    rc, out = _run(program, [(0, 0, ho, w)], 1, s, up, mid, 3 * ho * wo)
    assert rc == 0 and np.array_equal(out.reshape(ho, wo, 3), RO.imresize(img, s, up)), (img.shape, s, up, "width")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_down_both_passes_equal_the_restatement(program, s):
    """One and two output rows (the taps reflect more than once), 343 output pixels (two 340-pixel tiles in the width pass), rows of
    3 * 343 s bytes (several 1024-byte column tiles in the height pass, with a byte tail at x2 and x3)."""
    rng = np.random.default_rng(20 + s)
    for h in (s, 2 * s):
        _both_passes(program, rng.integers(0, 256, (h, 343 * s, 3), dtype=np.uint8), s, False)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_up_both_passes_equal_the_restatement(program, s):
    rng = np.random.default_rng(30 + s)
    for h, w in ((1, 1), (2, 343)):
        _both_passes(program, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), s, True)


@pytest.mark.parametrize("s,up", [(2, False), (3, False), (4, False), (3, True)])
def test_pooled_call_at_odd_offsets_touches_nothing_else(program, s, up):
    """Two images of one call per pass, sources and destinations at offsets that are no multiples of 4; every byte of the destination
    outside the two outputs keeps the program's fill value 9."""
    rng = np.random.default_rng(40 + s)
    imgs = [rng.integers(0, 256, (2 * s, 3 * s, 3), dtype=np.uint8), rng.integers(0, 256, (3 * s, 7 * s, 3), dtype=np.uint8)]
    for axis in (0, 1):
        srcs = imgs if axis == 0 else [_mid(im, s, up) for im in imgs]
        wants = [_mid(im, s, up) for im in imgs] if axis == 0 else [RO.imresize(im, s, up) for im in imgs]
        so = [1, _odd(1 + srcs[0].size)]
        do = [3, _odd(3 + wants[0].size)]
        pool = np.full(so[1] + srcs[1].size, 77, np.uint8)
        for o, im in zip(so, srcs):
            pool[o:o + im.size] = im.reshape(-1)
        nbytes = do[1] + wants[1].size + 5
        rc, out = _run(program, [(so[i], do[i]) + srcs[i].shape[:2] for i in range(2)], axis, s, up, pool, nbytes)
        want = np.full(nbytes, 9, np.uint8)
        for o, wimg in zip(do, wants):
            want[o:o + wimg.size] = wimg.reshape(-1)
        assert rc == 0 and np.array_equal(out, want), (s, up, axis)


def test_refused_descriptors_launch_nothing(program):
    """The refused calls of tests/test_resize_gpu.py: PESR_EINVAL (-1, 255 as an exit status) and not a byte written."""
    rng = np.random.default_rng(1)
    pool = rng.integers(0, 256, 8 * 10 * 3, dtype=np.uint8)
    wts = _weights(2, False)
    nbytes = 8 * 10 * 3 * 16
    for rows, axis, s, up in (([(0, 0, 8, 10)], 0, 5, 0),                                 # s outside {2, 3, 4}
                              ([(0, 0, 8, 10)], 0, 1, 1),
                              ([(0, 0, 8, 10)], 0, 3, 0),                                 # 8 rows do not divide by 3
                              ([(0, 0, 8, 10)], 1, 4, 0),                                 # 10 columns do not divide by 4
                              ([(0, 0, 8, 10), (0, 120, 0, 10)], 0, 2, 0),                # an empty image among valid ones
                              ([(0, 0, 8, 10)], 2, 2, 0)):                                # no such axis
        rc, out = _run(program, rows, axis, s, up, pool, nbytes, wts=wts)
        assert rc == 255 and (out == 9).all(), (rows, axis, s, up)
    rc, out = _run(program, [(0, 0, 8, 10)], 0, 2, 0, pool, nbytes, wts=wts)             # (the same call with valid arguments does run)
    assert rc == 0 and np.array_equal(out[:120].reshape(4, 10, 3), _mid(pool.reshape(8, 10, 3), 2, False)) and (out[120:] == 9).all()
