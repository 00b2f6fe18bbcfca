"""CPU: pesr_amd/csrc/degrade.hip compiled as plain C++ into a stand-alone program (tests/host_build.py: the lanes of a workgroup as
threads, __syncthreads as a barrier) and run on the host - the kernel, the descriptor checks and the grid walk as they are - against
the float64 restatement tests/degrade_oracle.py, bit for bit.  Nothing is loaded into Python; no GPU is involved."""
import numpy as np
import pytest

import degrade_oracle as DO
import host_build

STREAM = (1 << 64) - 3


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_build.build("degrade", tmp_path_factory.mktemp("degrade_host"))


def _bits(x):
    from pesr_amd._pool import f64_bits
    return f64_bits(x)


def _i64(q):
    return q - (1 << 64) if q >> 63 else q


def _run(program, rows, s, K, bank, pool, dst_bytes, n=None, n_kernels=None):
    bank = np.ascontiguousarray(bank, dtype=np.float64)
    head = np.array([len(rows) if n is None else n, s, K, len(bank) if n_kernels is None else n_kernels, bank.size, pool.size, dst_bytes],
                    dtype=np.int64)
    return host_build.run(program, [head.tobytes(), np.array(rows, dtype=np.int64).reshape(-1, 11).tobytes(), bank.tobytes(), pool.tobytes()])


def _bank(K):
    return np.stack([DO.gaussian_kernel(K, 0.3 * K + 0.4), DO.gaussian_kernel(K, 0.25 * K + 0.5, 0.1 * K + 0.3, 0.7)])


@pytest.mark.parametrize("s,K", [(2, 2), (3, 1), (3, 23), (4, 24)])
def test_entries_of_one_call_equal_the_restatement(program, s, K):
    """A 17s x 18s image that starts 5 bytes into the pool, four entries of one call: the whole image (2 x 2 tiles, three of them
    partial) with kernel 0 and no noise; the whole image again with kernel 1 and noise; a 5 x 7 window at the far corner (the
    clamp at two borders) without and with noise.  Every byte outside the four outputs keeps the program's fill value 9."""
    rng = np.random.default_rng(50 + s + K)
    H, W = 17 * s, 18 * s
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pool = np.concatenate([np.full(5, 77, np.uint8), img.reshape(-1)])
    bank = _bank(K)
    entries = [((0, 0, 17, 18), 0, 0.0, 0), ((0, 0, 17, 18), 1, 6.5, STREAM), ((12, 11, 5, 7), 1, 0.0, 0), ((12, 11, 5, 7), 0, 2.25, STREAM)]
    rows, wants, dof = [], [], 1
    for (y0, x0, h, w), ki, sig, q in entries:
        rows.append((5, dof, H, W, y0, x0, h, w, ki, _bits(sig), _i64(q)))
        wants.append((dof, DO.degrade(img, s, bank[ki], sig, q, (y0, x0, h, w))))
        dof += 3 * h * w + 2
    rc, out = _run(program, rows, s, K, bank, pool, dof)
    want = np.full(dof, 9, np.uint8)
    for o, wimg in wants:
        want[o:o + wimg.size] = wimg.reshape(-1)
    assert rc == 0 and np.array_equal(out, want)
    assert not np.array_equal(wants[0][1], wants[1][1]) and not np.array_equal(wants[2][1], wants[3][1])      # (the noise is seen)


def test_refused_calls_launch_nothing(program):
    """The refused calls of tests/test_degrade_gpu.py: PESR_EINVAL (-1, 255 as an exit status) and not a byte written."""
    rng = np.random.default_rng(1)
    pool = rng.integers(0, 256, 8 * 12 * 3, dtype=np.uint8)
    banks = {K: _bank(K) for K in (1, 2, 3, 4, 24)}

    def call(rows, s=2, K=2, n=None, n_kernels=2):
        return _run(program, rows, s, K, banks.get(K, banks[24]), pool, 4096, n=n, n_kernels=n_kernels)

    def row(H=8, W=12, y0=0, x0=0, h=4, w=6, kidx=0, sigma=0.0, q=0, so=0, dof=0):
        return (so, dof, H, W, y0, x0, h, w, kidx, _bits(sigma), q)

    refused = [call([row()], s=5, K=1),                          # s outside {2, 3, 4}
               call([row()], s=1, K=1),
               call([row()], s=2, K=3),                          # K of the wrong parity
               call([row(h=2, w=4)], s=3, K=2),
               call([row()], s=2, K=0),                          # K outside 1..24
               call([row()], s=2, K=26),
               call([row(h=2, w=4)], s=3, K=1),                  # 8 rows do not divide by 3
               call([row(H=8, W=10, h=2, w=2)], s=4, K=2),       # 10 columns do not divide by 4
               call([row(h=0)]),                                 # an empty window
               call([row(w=0)]),
               call([row(y0=1)]),                                # a window outside the LR grid: 1 + 4 > 4
               call([row(x0=1)]),
               call([row(y0=-1, h=2)]),
               call([row(x0=-1, w=2)]),
               call([row(kidx=2)]),                              # a kernel index outside the bank
               call([row(kidx=-1)]),
               call([row(kidx=1)], n_kernels=1),
               call([row(sigma=-1.0)]),                          # a negative or non-finite sigma_n
               call([row(sigma=float("inf"))]),
               call([row(sigma=float("nan"))]),
               call([row()], n=0),                               # n < 1
               call([row(), row(h=0, dof=72)])]                  # an invalid entry among valid ones
    for i, (rc, out) in enumerate(refused):
        assert rc == 255 and (out == 9).all(), i
    rc, out = call([row(sigma=3.0, q=5, kidx=1)])                # (the corrected call does run)
    want = DO.degrade(pool.reshape(8, 12, 3), 2, banks[2][1], 3.0, 5)
    assert rc == 0 and np.array_equal(out[:72].reshape(4, 6, 3), want) and (out[72:] == 9).all()
