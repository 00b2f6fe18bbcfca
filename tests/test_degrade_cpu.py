"""CPU: the classical degradation of docs/modes.md section 4j without a GPU - the float64 restatement (tests/degrade_oracle.py)
against torch's float64 convolution and against cases written out by hand, the noise generator, the host-side kernel maker and
DegradationSpec of pesr_amd/degrade.py, the entry points' flag checks, and the golden fixture that pins the restatement."""
import importlib.util
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _onehot(K, i, j):
    k = np.zeros((K, K))
    k[i, j] = 1.0
    return k


@pytest.mark.parametrize("s", [2, 3, 4])
def test_restatement_equals_torch_conv2d(s):
    """Without the rounding: replicate padding of (K-s)/2 before and K-s-(K-s)/2 ... the offset (s-K)/2 as padding, then a
    stride-s cross-correlation.  K < s would need a crop instead of a pad, K = s needs neither."""
    for n, K in enumerate((s, s + 2, 24 if s % 2 == 0 else 23)):
        img = _rand(5 * s, 7 * s, 10 * s + n)
        k = np.random.default_rng(50 + n).random((K, K))
        k = k / k.sum()
        want = DO.degrade(img, s, k, rounded=False)
        before = (K - s) // 2                      # taps start (K-s)/2 pixels before the block ...
        after = K - s - before                     # ... and end this many behind it (equal: K - s is even)
        x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
        x = F.pad(x, (before, after, before, after), mode="replicate")
        wt = torch.from_numpy(k)[None, None].expand(3, 1, K, K).contiguous()
        got = F.conv2d(x, wt, stride=s, groups=3)[0].permute(1, 2, 0).numpy()
        assert got.shape == want.shape == (5, 7, 3)
        assert np.abs(got - want).max() <= 1e-9, (s, K, np.abs(got - want).max())


def test_box_kernel_is_the_block_mean_with_ties_up_and_clamp():
    for s in (2, 4):
        box = np.full((s, s), 1.0 / (s * s))
        img = _rand(3 * s, 4 * s, s)
        mean = img.reshape(3, s, 4, s, 3).astype(np.float64).mean(axis=(1, 3))            # dyadic: exact
        assert np.array_equal(DO.degrade(img, s, box), np.floor(mean + 0.5).astype(np.uint8))
    # a tie goes up: the block (0, 0, 1, 1) has mean 0.5 -> 1
    blk = np.zeros((2, 2, 3), np.uint8)
    blk[1] = 1
    assert DO.degrade(blk, 2, np.full((2, 2), 0.25)).tolist() == [[[1, 1, 1]]]
    assert DO.degrade(blk, 2, np.full((2, 2), 0.25), rounded=False).tolist() == [[[0.5, 0.5, 0.5]]]
    # the clamp, both sides: weights that overshoot, and noise on black and white
    sharp = np.array([[2.0, -0.5], [-0.5, 0.0]])
    img = np.zeros((2, 4, 3), np.uint8)
    img[0, 0], img[0, 3], img[1, 2] = 255, 255, 255
    assert DO.degrade(img, 2, sharp).tolist() == [[[255] * 3, [0] * 3]]                  # 510 and -255 before the clamp
    for v in (0, 255):
        flat = np.full((8, 8, 3), v, np.uint8)
        out = DO.degrade(flat, 2, np.full((2, 2), 0.25), 30.0, 3)
        pre = DO.degrade(flat, 2, np.full((2, 2), 0.25), 30.0, 3, rounded=False)
        assert (pre < 0).any() or (pre > 255).any()
        assert np.array_equal(out, np.floor(np.clip(pre, 0, 255) + 0.5).astype(np.uint8)) and (out == v).any() and (out != v).any()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_one_hot_kernels_pick_the_named_pixel(s):
    img = _rand(6 * s, 5 * s, 20 + s)
    H, W = img.shape[:2]
    K = s + 4
    for i, j in ((0, 0), (K - 1, 0), (2, K - 1), (K // 2, K // 2)):
        out = DO.degrade(img, s, _onehot(K, i, j))
        for oy in range(6):
            for ox in range(5):
                r = min(max(s * oy + (s - K) // 2 + i, 0), H - 1)
                c = min(max(s * ox + (s - K) // 2 + j, 0), W - 1)
                assert np.array_equal(out[oy, ox], img[r, c]), (s, i, j, oy, ox)
    # a window of the image equals that part of the whole: the taps reach into the real image, not a clamped crop
    k = DO.gaussian_kernel(K, 0.7 * s)
    whole = DO.degrade(img, s, k)
    assert np.array_equal(DO.degrade(img, s, k, window=(1, 2, 4, 3)), whole[1:5, 2:5])


def test_one_lr_pixel_with_the_widest_kernel_has_every_tap_clamped():
    for s, K in ((2, 24), (3, 23), (4, 24)):
        img = _rand(s, s, 30 + s)
        k = np.random.default_rng(s).random((K, K))
        k /= k.sum()
        # every tap lands on one of the s x s pixels: fold the kernel onto them, in tap order
        acc = np.zeros(3)
        for i in range(K):
            for j in range(K):
                r = min(max(s * 0 + (s - K) // 2 + i, 0), s - 1)
                c = min(max((s - K) // 2 + j, 0), s - 1)
                acc = acc + k[i, j] * img[r, c].astype(np.float64)
        assert DO.degrade(img, s, k).shape == (1, 1, 3)
        assert np.array_equal(DO.degrade(img, s, k, rounded=False)[0, 0], acc)


def test_noise_first_values_are_pinned():
    assert DO.gauss(0, 4).tolist() == [0.54412841796875, -1.03558349609375, 0.668914794921875, 2.1968231201171875]
    assert DO.gauss(1, 4).tolist() == [0.471038818359375, -0.11328125, -1.078521728515625, 0.8679351806640625]
    assert DO.gauss(0, 3, first=1).tolist() == DO.gauss(0, 4).tolist()[1:]
    # the scalar form of the definition, in Python integers
    key = DO.splitmix64(2 ** 63 + 5)
    z = [DO.splitmix64((key + 3 * 9 + j) % 2 ** 64) for j in range(3)]
    S = sum((v >> sh) & 0xffff for v in z for sh in (0, 16, 32, 48))
    assert (2 * S - 786420) / 131072 == DO.gauss(2 ** 63 + 5, 10)[9]


def test_noise_moments_and_stream_independence():
    for q in (0, 1, 12345, 2 ** 63 + 5):
        g = DO.gauss(q, 1 << 20)
        print(f"q = {q}: mean {g.mean():+.5f}, std {g.std():.5f}, max |g| {np.abs(g).max():.3f}")
        assert abs(g.mean()) <= 0.005 and abs(g.std() - 1) <= 0.005 and np.abs(g).max() <= 6
    corr = np.corrcoef(DO.gauss(7, 1000), DO.gauss(8, 1000))[0, 1]
    print(f"corr(g(7, .), g(8, .)) = {corr:+.4f}")
    assert abs(corr) <= 0.1


def test_sigma_zero_skips_the_noise_term():
    img = _rand(8, 8, 4)
    k = DO.gaussian_kernel(4, 1.0)
    assert np.array_equal(DO.degrade(img, 2, k, 0.0, 99, rounded=False), DO.degrade(img, 2, k, rounded=False))
    assert not np.array_equal(DO.degrade(img, 2, k, 5.0, 99), DO.degrade(img, 2, k))
    assert not np.array_equal(DO.degrade(img, 2, k, 5.0, 99), DO.degrade(img, 2, k, 5.0, 100))


def test_gaussian_kernel_properties():
    from pesr_amd.degrade import gaussian_kernel, kernel_size, legal_kernel_size
    for K, s1, s2, th in ((24, 3.2, None, 0.0), (11, 1.6, None, 0.0), (23, 2.4, 0.9, 0.7), (10, 1.6, 0.4, 2.9), (1, 0.5, None, 0.0)):
        k = gaussian_kernel(K, s1, s2, th)
        assert k.dtype == np.float64 and k.shape == (K, K)
        assert abs(math.fsum(k.reshape(-1).tolist()) - 1.0) <= 1e-15
        assert np.array_equal(k, k[::-1, ::-1])                                           # a 180 degree turn
        assert np.array_equal(k, DO.gaussian_kernel(K, s1, s2, th))                       # product and restatement agree bit for bit
    # isotropic: the outer product of its row sums
    k = gaussian_kernel(15, 2.0)
    assert np.abs(k - np.outer(k.sum(axis=1), k.sum(axis=0))).max() <= 1e-15
    assert np.array_equal(k, k.T)
    # theta = pi / 2 swaps the axes; the long axis lies along x (columns) at theta = 0
    a, b = gaussian_kernel(13, 2.5, 0.8, 0.0), gaussian_kernel(13, 2.5, 0.8, math.pi / 2)
    assert np.abs(a.T - b).max() <= 1e-15 and np.abs(a - gaussian_kernel(13, 0.8, 2.5, math.pi / 2)).max() <= 1e-15
    assert a[6, 0] > a[0, 6]
    for s in (2, 3, 4):
        for sig in (0.0, 0.1, 0.2 * s, 0.8 * s, 1.6, 3.9, 4.0, 100.0):
            K = kernel_size(s, sig)
            assert legal_kernel_size(s, K) and DO.legal(s, K)
            assert K >= 6 * sig or K == (24 if s % 2 == 0 else 23)
            assert K - 2 < 1 or K - 2 < 6 * sig                                            # the smallest such
    assert [kernel_size(s, 0.8 * s) for s in (2, 3, 4)] == [10, 15, 20] and kernel_size(3, 1.6) == 11
    assert [kernel_size(s, 4.0) for s in (2, 3, 4)] == [24, 23, 24]
    with pytest.raises(ValueError):
        gaussian_kernel(5, 0.0)


class _CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def uniform(self, a, b):
        self.calls.append("uniform")
        return super().uniform(a, b)

    def getrandbits(self, k):
        self.calls.append("getrandbits")
        return super().getrandbits(k)


def test_degradation_spec_draw():
    from pesr_amd.degrade import DegradationSpec
    spec = DegradationSpec(0.8, 3.2, True, 25.0)
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    before = (random.getstate(), np.random.get_state()[1].tolist(), torch.random.get_rng_state().tolist())
    src = random.Random(11)
    src.random()
    a, b = random.Random(), random.Random()
    a.setstate(src.getstate())
    b.setstate(src.getstate())
    pa, pb = [spec.draw(a) for _ in range(20)], [spec.draw(b) for _ in range(20)]
    assert pa == pb and len(set(pa)) == 20
    assert before == (random.getstate(), np.random.get_state()[1].tolist(), torch.random.get_rng_state().tolist())   # only the rng it is handed
    for s1, s2, th, sn, q in pa:
        assert 0.8 <= s2 <= s1 <= 3.2 and 0 <= th < math.pi and 0 <= sn <= 25.0 and 0 <= q < 2 ** 64
    r = _CountingRandom(3)
    s1, s2, th, sn, q = DegradationSpec(0.8, 3.2, False, 0.0).draw(r)
    assert r.calls == ["uniform", "getrandbits"] and s2 == s1 and th == 0.0 and sn == 0.0
    r = _CountingRandom(3)
    DegradationSpec(0.8, 3.2, True, 1.0).draw(r)
    assert r.calls == ["uniform"] * 4 + ["getrandbits"]
    # the order: sigma1, (sigma2, theta), (sigma_n), q
    r, ref = random.Random(9), random.Random(9)
    s1 = ref.uniform(0.8, 3.2)
    s2 = ref.uniform(0.8, s1)
    th = ref.uniform(0.0, math.pi)
    sn = ref.uniform(0.0, 25.0)
    assert spec.draw(r) == (s1, s2, th, sn, ref.getrandbits(64))


def test_train_flags():
    T = _entry("train")
    a = T.build_parser().parse_args([])
    assert a.degradation == "bicubic" and a.blur_sigma == "" and a.blur_aniso is False and a.noise_sigma == 0.0
    assert T.degradation_spec(a) is None
    ok = ["--degradation", "classical", "--lr_from_hr", "true", "--gpu_pipeline", "true"]
    spec = T.degradation_spec(T.build_parser().parse_args(ok + ["--scale", "3"]))
    assert spec.sigma_lo == 0.2 * 3 and spec.sigma_hi == 0.8 * 3 and spec.aniso is False and spec.noise_hi == 0.0
    spec = T.degradation_spec(T.build_parser().parse_args(ok + ["--blur_sigma", "0.5,2", "--blur_aniso", "true", "--noise_sigma", "10"]))
    assert tuple(spec) == (0.5, 2.0, True, 10.0)
    # main() refuses before it touches a device
    for bad in (["--degradation", "classical"],
                ["--degradation", "classical", "--lr_from_hr", "true"],
                ["--degradation", "classical", "--gpu_pipeline", "true"],
                ok + ["--synthetic", "8"]):
        with pytest.raises(SystemExit, match=r"--degradation classical.*--lr_from_hr true --gpu_pipeline true and no --synthetic"):
            T.main(bad)
    for bad in ("1", "2,1", "0,1", "a,b", "1,2,3"):
        with pytest.raises(SystemExit, match="--blur_sigma"):
            T.main(ok + ["--blur_sigma", bad])
    with pytest.raises(SystemExit, match="noise"):
        T.main(ok + ["--noise_sigma", "-1"])


def test_test_flags():
    T = _entry("test")
    a = T.build_parser().parse_args([])
    assert a.degradation == "bicubic" and T.classical_kernel(a) is None
    with pytest.raises(SystemExit, match=r"--degradation classical.*--from_hr true"):
        T.main(["--degradation", "classical", "--blur_sigma", "1.6"])
    ok = ["--degradation", "classical", "--from_hr", "true"]
    k = T.classical_kernel(T.build_parser().parse_args(ok + ["--scale", "3", "--blur_sigma", "1.6"]))
    assert np.array_equal(k, DO.gaussian_kernel(11, 1.6))                                  # the BD row
    k = T.classical_kernel(T.build_parser().parse_args(ok + ["--scale", "4", "--blur_sigma", "2,1,0.5"]))
    assert np.array_equal(k, DO.gaussian_kernel(12, 2.0, 1.0, 0.5))
    for s, K in ((2, 2), (3, 1), (4, 2)):                                                  # the DN row: no blur
        k = T.classical_kernel(T.build_parser().parse_args(ok + ["--scale", str(s), "--noise_sigma", "30"]))
        assert k.shape == (K, K) and np.array_equal(k, np.full((K, K), 1.0 / (K * K)))
    for bad in ("1,2", "x", "-1", "1,0,0"):
        with pytest.raises(SystemExit, match="--blur_sigma"):
            T.main(ok + ["--blur_sigma", bad])
    with pytest.raises(SystemExit, match="--noise_sigma"):
        T.main(ok + ["--noise_sigma", "-3"])


def test_no_cpu_fallback():
    from pesr_amd import _lib
    from pesr_amd.degrade import degrade_pool_u8, degrade_u8
    img = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        degrade_u8(img, 2, np.full((2, 2), 0.25))
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        degrade_pool_u8(img.view(-1), [0], [(4, 4)], 2, np.full((1, 2, 2), 0.25), [0], [0.0], [0])


def test_golden_fixture_pins_the_restatement():
    g = np.load(os.path.join(ROOT, "tests", "golden", "gv15_degrade.npz"))
    n = 0
    while f"in{n}" in g:
        s, sigma_n, q, y0, x0, h, w = g[f"par{n}"].tolist()
        out = DO.degrade(g[f"in{n}"], int(s), g[f"k{n}"], sigma_n, int(q), (int(y0), int(x0), int(h), int(w)))
        assert out.dtype == np.uint8 and np.array_equal(out, g[f"out{n}"]), n
        n += 1
    assert n == 7
    # the file was written by tests/golden/make_golden_degrade.py: same inputs today
    spec = importlib.util.spec_from_file_location("make_golden_degrade", os.path.join(ROOT, "tests", "golden", "make_golden_degrade.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for i, (img, s, k, sigma_n, q, win) in enumerate(m.cases()):
        assert np.array_equal(img, g[f"in{i}"]) and np.array_equal(k, g[f"k{i}"]) and g[f"par{i}"][0] == s
