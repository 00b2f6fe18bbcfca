"""GPU: the classical degradation of docs/modes.md section 4j (pesr_amd/csrc/degrade.hip through the C ABI) against the float64
restatement of tests/degrade_oracle.py - BIT FOR BIT, no excused pixels: the order of operations is fixed and nothing is fused, so
kernel and restatement perform the same IEEE operations - and its users: GpuPatchSampler.from_hr(degradation=...),
train.py --degradation classical, test.py --degradation classical."""
import ctypes
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import degrade_oracle as DO
import resize_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (5 * x + 2 * y) // 2 % 256], axis=2).astype(np.uint8)


def _kmax(s):
    return 24 if s % 2 == 0 else 23


def _ksizes(s):
    """K = s, the smallest legal K >= 6 * 0.8 * s (the default training range's), the largest legal K."""
    from pesr_amd.degrade import kernel_size
    return [s, kernel_size(s, 0.8 * s), _kmax(s)]


def _kernel(K, seed):
    """A blur kernel for K: the box at seed 0, an anisotropic Gaussian otherwise."""
    if seed == 0:
        return np.full((K, K), 1.0 / (K * K))
    r = random.Random(seed)
    return DO.gaussian_kernel(K, r.uniform(0.5, 1.0) * max(K / 6.0, 0.5), r.uniform(0.2, 0.5) * max(K / 6.0, 0.5), r.uniform(0, np.pi))


def _report(got, want, what, near):
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = np.argwhere(diff != 0)
    # a mismatch with near-ties > 0 points at a contracted multiply-add, one with 0 at indexing
    pytest.fail(f"{what}: {len(bad)} bytes differ (max {np.abs(diff).max()}), first at {bad[0].tolist()}; restatement values within "
                f"1e-9 of a tie without being one: {near}")


def _check(img, s, k, what, sigma_n=0.0, q=0):
    from pesr_amd.degrade import degrade_u8
    want = DO.degrade(img, s, k, sigma_n, q)
    got = degrade_u8(torch.from_numpy(img).to(DEV), s, k, sigma_n, q).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    if not torch.equal(got, torch.from_numpy(want)):
        _report(got.numpy(), want, f"{what} x{s} K={k.shape[0]} sigma_n={sigma_n} {img.shape}", DO.near_ties(img, s, k, sigma_n, q))


# LR sizes (h, w): one pixel (every tap clamped), below / exactly / above one 16 x 16 tile in either axis, several tiles in one axis only
SIZES = [(1, 1), (2, 2), (5, 7), (16, 16), (17, 33), (3, 40)]


@pytest.mark.parametrize("s", [2, 3, 4])
def test_whole_images_bit_exact(s):
    for ki, K in enumerate(_ksizes(s)):
        for n, (h, w) in enumerate(SIZES):
            noisy = (n + ki) % 2 == 1
            _check(_rand(s * h, s * w, 100 * s + 10 * ki + n), s, _kernel(K, ki * 7 + n if K > s else 0), "random",
                   12.5 if noisy else 0.0, 1000 + n)
        _check(_ramp(s * 24, s * 31), s, _kernel(K, 0), "ramp, box")            # the tie-heavy case at x2 / x4
        _check(_ramp(s * 24, s * 31), s, _kernel(K, 3), "ramp")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_clamp_cases_bit_exact(s):
    from pesr_amd.degrade import degrade_u8
    K = _kmax(s)
    for v in (0, 255):
        flat = np.full((s * 6, s * 5, 3), v, np.uint8)
        _check(flat, s, _kernel(s, 0), f"all-{v} + noise", 30.0, 2 ** 63 + 5)
        out = degrade_u8(torch.from_numpy(flat).to(DEV), s, _kernel(s, 0), 30.0, 2 ** 63 + 5)
        assert bool((out == v).any()) and bool((out != v).any())                 # the clamp was hit, and not everywhere
    img = np.zeros((s * 20, s * 20, 3), np.uint8)
    img[s * 3:s * 8, s * 4:s * 9] = 255
    img[s * 12:, :s * 5] = 255
    _check(img, s, _kernel(K, 5), "blocks")
    _check(img, s, _kernel(K, 5), "blocks + noise", 30.0, 9)
    # weights that overshoot on both sides (not a blur: the API takes any kernel)
    sharp = np.zeros((s + 2, s + 2))
    sharp[1:-1, 1:-1] = 3.0 / (s * s)
    sharp[0, 0] = sharp[-1, -1] = -1.0
    _check(img, s, sharp, "overshoot")
    # one-hot kernels pick the named HR pixel
    for i, j in ((0, 0), (K - 1, 2), (K // 2, K - 1)):
        onehot = np.zeros((K, K))
        onehot[i, j] = 1.0
        _check(_rand(s * 9, s * 18, 40 + i), s, onehot, f"one-hot ({i}, {j})")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_one_launch_many_entries(s):
    from pesr_amd.degrade import degrade_pool_u8, degrade_u8, kernel_size
    K = kernel_size(s, 0.8 * s)
    imgs = [_rand(s * h, s * w, 200 + n) for n, (h, w) in enumerate([(20, 23), (1, 1), (8, 3), (3, 40)])]
    # images back to back with odd gaps: offsets that are not multiples of 4
    offs, flat, pos = [], [], 0
    for n, im in enumerate(imgs):
        gap = [1, 2, 3, 5][n]
        flat.append(np.full(gap, 77, np.uint8)); pos += gap
        offs.append(pos); flat.append(im.reshape(-1)); pos += im.size
    assert any(o % 4 for o in offs)
    pool = torch.from_numpy(np.concatenate(flat)).to(DEV)
    # (image, window): the four corners and the interior of image 0, then every image whole
    ents = [(0, (0, 0, 5, 6)), (0, (0, 16, 7, 7)), (0, (14, 0, 6, 5)), (0, (15, 17, 5, 6)), (0, (6, 5, 9, 11)), (0, (2, 3, 17, 18)),
            (0, (0, 0, 20, 23)), (1, (0, 0, 1, 1)), (2, (0, 0, 8, 3)), (3, (0, 0, 3, 40))]
    n = len(ents)
    bank = np.stack([_kernel(K, 11 + e) for e in range(n)])
    kidx = [(3 * e + 1) % n for e in range(n)]                                     # a permutation: every entry another kernel
    assert sorted(kidx) == list(range(n))
    sig = [0.0 if e % 3 == 0 else 4.0 + e for e in range(n)]
    qs = [2 ** 64 - 1 - e * 12345678901 for e in range(n)]
    out, ooffs, oshapes = degrade_pool_u8(pool, [offs[i] for i, _ in ents], [imgs[i].shape[:2] for i, _ in ents], s, bank, kidx, sig, qs,
                                          windows=[w for _, w in ents])
    assert out.dtype == torch.uint8 and out.dim() == 1 and oshapes == [(w[2], w[3]) for _, w in ents]
    assert ooffs[-1] + 3 * oshapes[-1][0] * oshapes[-1][1] == out.numel()
    for e, (i, win) in enumerate(ents):
        y0, x0, h, w = win
        got = out[ooffs[e]:ooffs[e] + 3 * h * w].view(h, w, 3).cpu()
        want = DO.degrade(imgs[i], s, bank[kidx[e]], sig[e], qs[e], win)
        if not torch.equal(got, torch.from_numpy(want)):
            _report(got.numpy(), want, f"entry {e} x{s} image {i} window {win}", DO.near_ties(imgs[i], s, bank[kidx[e]], sig[e], qs[e], win))
        whole = (y0, x0, h, w) == (0, 0) + tuple(v // s for v in imgs[i].shape[:2])
        if whole or sig[e] == 0:          # (the noise of a window is indexed inside the window)
            one = degrade_u8(torch.from_numpy(imgs[i]).to(DEV), s, bank[kidx[e]], sig[e], qs[e]).cpu()
            assert torch.equal(got, one[y0:y0 + h, x0:x0 + w]), e


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def test_invalid_arguments_return_einval_and_launch_nothing():
    from pesr_amd import _lib
    from pesr_amd.degrade import degrade_u8
    L = _lib.lib()
    src = torch.from_numpy(_rand(8, 12, 1)).to(DEV)
    dst = torch.full((4096,), 9, dtype=torch.uint8, device=DEV)
    banks = {K: torch.from_numpy(np.stack([_kernel(K, 0), _kernel(K, 2)])).to(DEV) for K in (1, 2, 3, 4, 24)}
    stream = torch.cuda.current_stream().cuda_stream

    def call(rows, s=2, K=2, n=None, n_kernels=2):
        d = np.array(rows, dtype=np.int64).reshape(-1, 11)
        dd = torch.from_numpy(d).to(DEV)
        return L.pesr_degrade_u8(src.data_ptr(), dst.data_ptr(), d.ctypes.data_as(ctypes.c_void_p), dd.data_ptr(), len(d) if n is None else n,
                                 s, K, banks.get(K, banks[24]).data_ptr(), n_kernels, stream)

    def row(H=8, W=12, y0=0, x0=0, h=4, w=6, kidx=0, sigma=0.0, q=0, so=0, dof=0):
        return (so, dof, H, W, y0, x0, h, w, kidx, _bits(sigma), q)

    assert call([row()], s=5, K=1) == -1                          # s outside {2, 3, 4}
    assert call([row()], s=1, K=1) == -1
    assert call([row()], s=2, K=3) == -1                          # K of the wrong parity
    assert call([row(h=2, w=4)], s=3, K=2) == -1
    assert call([row()], s=2, K=0) == -1                          # K outside 1..24
    assert call([row()], s=2, K=26) == -1
    assert call([row(h=2, w=4)], s=3, K=1) == -1                  # 8 rows do not divide by 3
    assert call([row(H=8, W=10, h=2, w=2)], s=4, K=2) == -1       # 10 columns do not divide by 4
    assert call([row(h=0)]) == -1                                 # an empty window
    assert call([row(w=0)]) == -1
    assert call([row(y0=1)]) == -1                                # a window outside the LR grid: 1 + 4 > 4
    assert call([row(x0=1)]) == -1
    assert call([row(y0=-1, h=2)]) == -1
    assert call([row(x0=-1, w=2)]) == -1
    assert call([row(kidx=2)]) == -1                              # a kernel index outside the bank
    assert call([row(kidx=-1)]) == -1
    assert call([row(kidx=1)], n_kernels=1) == -1
    assert call([row(sigma=-1.0)]) == -1                          # a negative or non-finite sigma_n
    assert call([row(sigma=float("inf"))]) == -1
    assert call([row(sigma=float("nan"))]) == -1
    assert call([row()], n=0) == -1                               # n < 1
    assert call([row(), row(h=0, dof=72)]) == -1                  # an invalid entry among valid ones
    torch.cuda.synchronize()
    assert bool((dst == 9).all())                                 # nothing ran
    assert call([row(sigma=3.0, q=5, kidx=1)]) == 0               # (the corrected call does run)
    torch.cuda.synchronize()
    want = DO.degrade(src.cpu().numpy(), 2, _kernel(2, 2), 3.0, 5)
    assert torch.equal(dst[:72].cpu().view(4, 6, 3), torch.from_numpy(want)) and bool((dst[72:] == 9).all())
    for s, k in ((5, _kernel(1, 0)), (2, _kernel(3, 0)), (3, _kernel(3, 0)), (2, np.full((26, 26), 1 / 676))):
        with pytest.raises(_lib.PesrHipError):
            degrade_u8(src, s, k)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        degrade_u8(src.cpu(), 2, _kernel(2, 0))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_gpu_patch_sampler_with_a_degradation_spec(s):
    from data import augment
    from pesr_amd.degrade import DegradationSpec, kernel_size
    from pesr_amd.input_pipeline import GpuPatchSampler
    hrs = [_rand(h, w, 300 + n) for n, (h, w) in enumerate(((11 * s + 1, 9 * s + s - 1), (8 * s, 13 * s), (9 * s + 1, 8 * s)))]
    crops = [DO.modcrop(h, s) for h in hrs]
    spec = DegradationSpec(0.2 * s, 0.8 * s, True, 10.0)
    K = kernel_size(s, spec.sigma_hi)
    samp = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=spec)
    plain = GpuPatchSampler.from_hr(hrs, DEV, scale=s)
    assert samp.lr_pool is None and [tuple(x) for x in samp.lr_shapes] == [(c.shape[0] // s, c.shape[1] // s, 3) for c in crops]
    assert torch.equal(samp.hr_pool, plain.hr_pool) and list(samp.hr_off) == list(plain.hr_off)
    P = 6
    rng = random.Random(4)
    picks = [(b % 3, (b * 2) % (crops[b % 3].shape[0] // s - P + 1), (b * 3) % (crops[b % 3].shape[1] // s - P + 1), b % 8) + spec.draw(rng)
             for b in range(16)]
    assert {p[3] for p in picks} == set(range(8))                        # all 8 augmentations
    picks[5] = picks[5][:7] + (0.0,) + picks[5][8:]                      # one sample without noise
    for nhwc in (False, True):
        lr, hr = samp.assemble(picks, P, nhwc=nhwc)
        _, hr_plain = plain.assemble([p[:4] for p in picks], P, nhwc=nhwc)
        assert torch.equal(hr, hr_plain) and lr.shape == (16, 3, P, P) and lr.is_contiguous(memory_format=torch.channels_last) == nhwc
        for b, (i, y, x, aug, s1, s2, th, sn, q) in enumerate(picks):
            win = DO.degrade(crops[i], s, DO.gaussian_kernel(K, s1, s2, th), sn, q, (y, x, P, P))
            l, h = augment(win, crops[i][s * y:s * (y + P), s * x:s * (x + P)], aug)
            assert torch.equal(lr[b].cpu(), torch.from_numpy(l.transpose(2, 0, 1).astype(np.float32))), (nhwc, b)
            assert torch.equal(hr[b].cpu(), torch.from_numpy(h.transpose(2, 0, 1).astype(np.float32))), (nhwc, b)
    # draw / draw_for: the crop as without a spec, then the spec's draw, from the same stream
    a, b = random.Random(2), random.Random(2)
    got = samp.draw_for([2, 0, 1], P, a)
    for pick, i in zip(got, [2, 0, 1]):
        h, w, _ = samp.lr_shapes[i]
        assert pick == (i, b.randint(0, h - P), b.randint(0, w - P), b.randint(0, 7)) + spec.draw(b)
    assert a.getstate() == b.getstate() and all(len(p) == 9 for p in samp.draw(5, P, a))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_gpu_patch_sampler_without_a_spec_is_unchanged(s):
    """degradation=None: the pools and the outputs of the existing constructor, fed the bicubic restatement's LR images."""
    from pesr_amd.input_pipeline import GpuPatchSampler
    hrs = [_rand(h, w, 300 + n) for n, (h, w) in enumerate(((11 * s + 1, 9 * s + s - 1), (8 * s, 13 * s), (9 * s + 1, 8 * s)))]
    crops = [RO.modcrop(h, s) for h in hrs]
    lrs = [RO.imresize(c, s, False) for c in crops]
    samp = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=None)
    old = GpuPatchSampler(lrs, crops, DEV, scale=s)
    assert samp.degradation is None and old.degradation is None
    assert torch.equal(samp.lr_pool, old.lr_pool) and torch.equal(samp.hr_pool, old.hr_pool)
    assert list(samp.lr_off) == list(old.lr_off) and list(samp.hr_off) == list(old.hr_off)
    assert [tuple(x) for x in samp.lr_shapes] == [tuple(x) for x in old.lr_shapes]
    P = 6
    a, b = random.Random(3), random.Random(3)
    picks = samp.draw(16, P, a)
    want = []
    for _ in range(16):                                                  # today's draw order: image, y, x, augmentation
        i = b.randrange(3)
        want.append((i, b.randint(0, lrs[i].shape[0] - P), b.randint(0, lrs[i].shape[1] - P), b.randint(0, 7)))
    assert picks == want and samp.draw_for([1, 2], P, a) == old.draw_for([1, 2], P, b)
    for nhwc in (False, True):
        for x, y in zip(samp.assemble(picks, P, nhwc=nhwc), old.assemble(picks, P, nhwc=nhwc)):
            assert torch.equal(x, y)


# ---- entry points, each in a fresh interpreter -------------------------------------------------------------------------------
TRAIN_PROG = """
import importlib.util, os, random, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({root!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
def run(tag, epochs, extra=()):
    print("RUN_" + tag, flush=True)
    random.seed(1); np.random.seed(1); torch.manual_seed(1)          # the Generator's initialisation
    Tm.main(["--num_channels", "16", "--num_blocks", "1", "--patch_size", "16", "--batch_size", "4", "--max_iters", "2", "--phase", "pretrain",
             "--train_dataset", "Toy", "--valid_dataset", "Toy", "--num_repeats", "2", "--degradation", "classical", "--blur_aniso", "true",
             "--noise_sigma", "10", "--lr_from_hr", "true", "--gpu_pipeline", "true", "--num_epochs", str(epochs),
             "--check_point", os.path.join({base!r}, tag)] + list(extra))
{runs}
print("ENTRY_OK")
"""


def _toy_folders(tmp_path, sizes):
    from PIL import Image
    rng = np.random.RandomState(8)
    for sub, szs in (("train", sizes), ("valid", [(41, 47), (49, 44)])):
        d = tmp_path / "data" / "origin" / sub / "Toy" / "HR"
        d.mkdir(parents=True)
        for i, (h, w) in enumerate(szs):
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(d / f"{i}.png")


def _run_train(tmp_path, runs):
    prog = TRAIN_PROG.format(root=ROOT, base=str(tmp_path / "ck"), runs=runs)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return {m.group(1): m.group(2) for m in re.finditer(r"RUN_(\w+)\n(.*?)(?=RUN_|ENTRY_OK)", r.stdout, flags=re.S)}


def test_train_entrypoint_classical(tmp_path):
    _toy_folders(tmp_path, [(60, 67), (54, 57), (64, 60), (57, 72)])
    out = _run_train(tmp_path, 'run("a", 1, ["--scale", "3"])')["a"]
    m = re.search(r"Epoch \[1/1\] lr \S+\s+l1 (\S+)", out)
    assert m and np.isfinite(float(m.group(1))) and float(m.group(1)) > 0, out[-2000:]
    m = re.search(r"Finish valid \[1/1\]\. PSNR: ([-\d.]+)dB", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    assert (tmp_path / "ck" / "a" / "pretrain" / "best_model.pt").exists()


def test_train_entrypoint_classical_resume_is_bit_identical(tmp_path):
    """An uninterrupted 2-epoch run against one stopped after epoch 1 and resumed with --resume auto: the per-sample kernels and noise
    streams come from the GPU loader's stream, which the training state already holds."""
    _toy_folders(tmp_path, [(70, 75), (66, 81), (80, 68), (72, 72)])
    st = '["--save_state_every", "1", "--resume", "auto", "--hip_graph", "false"]'
    out = _run_train(tmp_path, f'run("full", 2, {st})\nrun("cut", 1, {st})\nrun("cut", 2, {st})')
    assert "Epoch [2/2]" in out["full"] and re.search(r"^resume: .*epoch 1 done, going on with epoch 2", out["cut"], flags=re.M), out["cut"][-1500:]
    full, cut = (tmp_path / "ck" / t / "pretrain" for t in ("full", "cut"))
    assert (full / "best_model.pt").read_bytes() == (cut / "best_model.pt").read_bytes()
    sa, sb = (torch.load(p / "train_state.pt", map_location="cpu", weights_only=False) for p in (full, cut))
    assert sa["epoch"] == sb["epoch"] == 2 and sa["best_psnr"] == sb["best_psnr"]
    for k in sa["G"]:
        assert torch.equal(sa["G"][k], sb["G"][k]), k
    assert sa["rng"][0]["gpu_loader"] == sb["rng"][0]["gpu_loader"]


def _host_psnr_y(a, b):
    """utils.compute_PSNR's host formula on two uint8 HWC arrays."""
    coef = np.array([65.738, 129.057, 25.064]) / 256.0
    ya = np.clip(np.dot(a.astype(np.float64), coef) + 16, 0, 255).round()
    yb = np.clip(np.dot(b.astype(np.float64), coef) + 16, 0, 255).round()
    return 20 * np.log10(255 / np.sqrt(np.mean((ya - yb) ** 2)))


TEST_PROG = """
import importlib.util, os, sys
sys.path.insert(0, {root!r})
spec = importlib.util.spec_from_file_location("entry_test", os.path.join({root!r}, "test.py"))
T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
T.main({args!r})
print("ENTRY_OK")
"""


def test_test_entrypoint_classical(tmp_path):
    """test.py --from_hr true --degradation classical --blur_sigma 1.6 --scale 3 (the BD row), then the DN row's flags at x2."""
    import importlib.util
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    spec = importlib.util.spec_from_file_location("entry_test_classical", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    for s, flags, kern, sigma_n, seed in ((3, ["--blur_sigma", "1.6"], DO.gaussian_kernel(11, 1.6), 0.0, 0),
                                          (2, ["--noise_sigma", "30", "--degrade_seed", "7"], np.full((2, 2), 0.25), 30.0, 7)):
        hrs = {"a.png": _ramp(12 * s + 1, 10 * s + s - 1), "b.png": _rand(9 * s, 14 * s, 5)}
        for name, im in hrs.items():
            Image.fromarray(im).save(base / "HR" / name)
        torch.save(gen_sd_scaled(16, 1, s, seed=3), tmp_path / f"g{s}.pt")
        args = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / f"g{s}.pt"), "--num_channels", "16", "--num_blocks", "1", "--scale", str(s),
                "--from_hr", "true", "--degradation", "classical", "--save_path", str(tmp_path / f"out{s}")] + flags
        r = subprocess.run([sys.executable, "-c", TEST_PROG.format(root=ROOT, args=args)], capture_output=True, text=True, timeout=300,
                           cwd=str(tmp_path))
        assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        for n, (name, im) in enumerate(hrs.items()):
            hr = DO.modcrop(im, s)
            lr = DO.degrade(hr, s, kern, sigma_n, seed + n)
            sr = np.asarray(Image.open(tmp_path / f"out{s}" / "Toy" / name).convert("RGB"))
            assert sr.shape == hr.shape                                       # PNGs at (mod-cropped) HR size
            m = re.search(re.escape(name) + r": PSNR-Y ([-\d.]+|inf) dB, bicubic ([-\d.]+|inf) dB", r.stdout)
            assert m, r.stdout
            bic = RO.imresize(lr, s, True)                                    # the "bicubic" column: bicubic x s of the DEGRADED LR
            want_sr, want_bic = _host_psnr_y(sr, hr), _host_psnr_y(bic, hr)
            print(f"x{s} {name}: printed {m.group(1)} / {m.group(2)}, host formula {want_sr!r} / {want_bic!r}")
            assert abs(float(m.group(1)) - want_sr) <= 1e-9 and abs(float(m.group(2)) - want_bic) <= 1e-9
            # the LR image fed to the model is the restatement's, bit for bit
            a = T.build_parser().parse_args(args)
            lr_t, hr_t, bic_t = T.lr_from_hr(im, s, DEV, T.classical_kernel(a), a.noise_sigma, a.degrade_seed + n)
            assert torch.equal(lr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(lr))
            assert torch.equal(bic_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(bic))
            assert torch.equal(hr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(np.ascontiguousarray(hr)))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_lr_image_is_the_composition_of_its_steps(s):
    """degrade.lr_image_u8 (one-entry degrade_chain_pool_u8, the JPEG step in place on the chain's pool) against degrade_u8, then
    resize_jitter_u8, then jpeg_u8, with the noise placed by hand: in the degrade launch without a jitter, in the jitter's second
    resize with one.  All eight subsets of {noise, jitter, JPEG}; the 48 x 36 HR image gives LR sides 24 x 18, 16 x 12 and 12 x 9:
    partial 8 x 8 and 16 x 16 JPEG blocks at 4:2:0.  Without a kernel: the bicubic resize, then the JPEG step when asked."""
    from pesr_amd.degrade import degrade_u8, gaussian_kernel, kernel_size, lr_image_u8, resize_jitter_u8
    from pesr_amd.jpeg import jpeg_u8
    from pesr_amd.resize import imresize_u8
    hr = torch.from_numpy(_rand(48, 36, 300 + s)).to(DEV)
    k = gaussian_kernel(kernel_size(s, 2.0), 2.0, 1.1, 0.6)
    for case in range(8):
        sigma_n, jitter, q = (6.0 if case & 1 else 0.0), ((0.37, 2, 1) if case & 2 else None), (40 if case & 4 else 0)   # (box, bilinear)
        want = degrade_u8(hr, s, k, 0.0 if jitter else sigma_n, 77)
        if jitter:
            want = resize_jitter_u8(want, jitter[0], jitter[1], jitter[2], sigma_n, 77)
        if q:
            want = jpeg_u8(want, q, True)
        got = lr_image_u8(hr, s, k, sigma_n, 77, jitter, q, True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (48 // s, 36 // s, 3)
        assert torch.equal(got, want), (s, case)
    bic = imresize_u8(hr, s, up=False)
    assert torch.equal(lr_image_u8(hr, s), bic)
    for chroma420 in (True, False):
        assert torch.equal(lr_image_u8(hr, s, jpeg_q=40, jpeg_420=chroma420), jpeg_u8(bic, 40, chroma420))
