"""GPU: the any-size resize of docs/modes.md section 4m (pesr_amd/csrc/resize_to.hip through the C ABI) against the float64
restatement of tests/resize_to_oracle.py - BIT FOR BIT, no excused pixels: the order of operations is fixed and nothing is fused, so
kernel and restatement perform the same IEEE operations - and its users: the resize jitter of GpuPatchSampler.from_hr, the loader's
resume, test.py --resize_jitter, train.py --resize_jitter."""
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
import jpeg_oracle as JO
import resize_oracle as RO
import resize_to_oracle as RT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")

# (input h x w, output h x w): single pixels, odd sizes, more than one workgroup's row segment (256 output pixels in the width pass,
# 1024 bytes in the height pass) in both directions, the 8:1 and 1:8 limits
CASES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 7), (1, 1)), ((9, 13), (4, 29)), ((40, 2), (5, 16)), ((3, 345), (7, 100)),
         ((7, 100), (3, 345)), ((48, 48), (33, 61)), ((48, 48), (6, 6)), ((6, 6), (48, 48))]


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ramp(h, w):
    return (np.arange(h * w * 3).reshape(h, w, 3) % 256).astype(np.uint8)             # the tie-heavy integer ramp


def _blocks(h, w):
    """Black and white blocks three pixels wide: the cubic's overshoot leaves [0, 255] on both sides."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((y // 3) + (x // 3)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _report(got, want, what, ties):
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = np.argwhere(diff != 0)
    pytest.fail(f"{what}: {len(bad)} bytes differ (max {np.abs(diff).max()}), first at {bad[0].tolist()}; {ties} near-ties in the restatement")


def _check(img, size, method, what):
    from pesr_amd.resize import imresize_to_u8
    want = RT.resize(img, size, method)
    got = imresize_to_u8(torch.from_numpy(img).to(DEV), size, method).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    if not torch.equal(got, torch.from_numpy(want)):
        _report(got.numpy(), want, f"{what} {method} {img.shape[:2]} -> {size}", RT.near_ties(img, size, method))


@pytest.mark.parametrize("method", RT.METHODS)
def test_every_case_of_the_table_bit_exact(method):
    for n, ((h, w), size) in enumerate(CASES):
        _check(_rand(h, w, 100 + n), size, method, "random")
        _check(_ramp(h, w), size, method, "ramp")
        _check(_blocks(h, w), size, method, "blocks")
        for v in (0, 255):
            _check(np.full((h, w, 3), v, np.uint8), size, method, f"flat {v}")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_integer_factors_equal_the_fixed_factor_kernels(s):
    from pesr_amd.resize import imresize_to_u8, imresize_u8
    for img in (_rand(12 * s, 17 * s, s), _ramp(12 * s, 17 * s), _blocks(12 * s, 17 * s)):
        t = torch.from_numpy(img).to(DEV)
        assert torch.equal(imresize_to_u8(t, (12, 17)), imresize_u8(t, s, up=False))
        assert torch.equal(imresize_to_u8(t, (12 * s * s, 17 * s * s)), imresize_u8(t, s, up=True))
    for method in RT.METHODS:                               # and the identity at equal size
        assert torch.equal(imresize_to_u8(t, (12 * s, 17 * s), method), t)


def test_one_pooled_call_equals_the_per_image_calls():
    """Five entries in one call: windows of two images that start 5 and 3 bytes off a multiple of 4 (strides above the widths),
    different sizes and filters, noise on three of them."""
    from pesr_amd.resize import imresize_to_pool_u8, imresize_to_u8
    a, b = _rand(24, 40, 1), _rand(31, 19, 2)
    pool = torch.from_numpy(np.concatenate([np.full(5, 77, np.uint8), a.reshape(-1), np.full(2, 78, np.uint8), b.reshape(-1)])).to(DEV)
    base = {0: (5, a, 40), 1: (5 + a.size + 2, b, 19)}
    wins = [(0, 0, 0, 15, 17, (7, 30), "bicubic", 0.0, 0), (0, 0, 17, 24, 23, (9, 5), "bilinear", 6.5, 12345),
            (0, 16, 1, 8, 9, (11, 13), "box", 2.25, (1 << 64) - 3), (1, 3, 2, 28, 16, (28, 16), "bicubic", 30.0, 1 << 63),
            (1, 0, 0, 31, 19, (4, 150), "bilinear", 0.0, 9)]
    offs = [base[i][0] + 3 * (y0 * base[i][2] + x0) for i, y0, x0, *_ in wins]
    out, ooffs, oshapes = imresize_to_pool_u8(pool, offs, [(h, w) for _, _, _, h, w, *_ in wins], [sz for *_, sz, _, _, _ in wins],
                                              [m for *_, m, _, _ in wins], strides=[base[i][2] for i, *_ in wins],
                                              noise_sigma=[sg for *_, sg, _ in wins], noise_stream=[q for *_, q in wins])
    assert oshapes == [sz for *_, sz, _, _, _ in wins] and ooffs == [int(v) for v in np.cumsum([0] + [3 * h * w for h, w in oshapes])[:-1]]
    assert out.numel() == sum(3 * h * w for h, w in oshapes)
    for (i, y0, x0, h, w, (ho, wo), m, sg, q), oo in zip(wins, ooffs):
        win = np.ascontiguousarray(base[i][1][y0:y0 + h, x0:x0 + w])
        got = out[oo:oo + 3 * ho * wo].view(ho, wo, 3).cpu()
        want = RT.resize(win, (ho, wo), m, sg, q)
        if not torch.equal(got, torch.from_numpy(want)):
            _report(got.numpy(), want, f"pooled {m} window {(y0, x0, h, w)} -> {(ho, wo)}", RT.near_ties(win, (ho, wo), m, sg, q))
        if sg == 0:
            assert torch.equal(got, imresize_to_u8(torch.from_numpy(win).to(DEV), (ho, wo), m).cpu())
        else:
            assert not np.array_equal(want, RT.resize(win, (ho, wo), m))              # (the noise is there)


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def test_invalid_arguments_return_einval_and_launch_nothing():
    from pesr_amd import _lib
    from pesr_amd.resize import imresize_to_pool_u8, imresize_to_u8, resize_table
    L = _lib.lib()
    img = _rand(8, 8, 3)
    src = torch.from_numpy(img).to(DEV)
    dst = torch.full((4096,), 9, dtype=torch.uint8, device=DEV)
    first, w = resize_table(8, 4, "bicubic")
    T = w.shape[1]
    table = np.concatenate([first, np.ascontiguousarray(w.T).reshape(-1).view(np.int64)])
    tab = torch.from_numpy(table).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rows, axis, n=None, words=None):
        d = np.array(rows, dtype=np.int64).reshape(-1, 12)
        dd = torch.from_numpy(d).to(DEV)
        return L.pesr_resize_to_u8_pass(src.data_ptr(), dst.data_ptr(), d.ctypes.data_as(ctypes.c_void_p), dd.data_ptr(), len(d) if n is None else n,
                                        axis, tab.data_ptr(), table.size if words is None else words, stream)

    def row(axis, so=0, ss=8, do=0, ds=None, hi=8, wi=8, ho=None, wo=None, at=0, taps=T, sigma=0.0, q=0):
        ho, wo = (4 if axis == 0 else 8) if ho is None else ho, (8 if axis == 0 else 4) if wo is None else wo
        return (so, ss, do, wo if ds is None else ds, hi, wi, ho, wo, at, taps, _bits(sigma), q)

    for axis in (0, 1):
        assert call([row(axis)], axis, n=0) == -1 and call([row(axis)], axis, n=-2) == -1                    # n < 1
        assert call([row(axis, hi=0)], axis) == -1 and call([row(axis, wi=0)], axis) == -1                   # a side < 1
        assert call([row(axis, ho=0)], axis) == -1 and call([row(axis, wo=0)], axis) == -1
        assert call([row(axis, ss=7)], axis) == -1 and call([row(axis, ds=3)], axis) == -1                   # a stride below the width
        assert call([row(axis, so=-1)], axis) == -1 and call([row(axis, do=-1)], axis) == -1                 # a negative offset
        assert call([row(axis, taps=0)], axis) == -1 and call([row(axis, taps=33)], axis) == -1              # T outside 1 .. 32
        assert call([row(axis, at=-1)], axis) == -1 and call([row(axis, at=1)], axis) == -1                  # a table outside the buffer
        assert call([row(axis)], axis, words=table.size - 1) == -1
        for sigma in (-1.0, float("nan"), float("inf")):
            assert call([row(axis, sigma=sigma)], axis) == -1
        assert call([row(axis), row(axis, hi=0)], axis) == -1                                                # an invalid entry after a valid one
    assert call([row(0, hi=33)], 0) == -1 and call([row(0, hi=1, ho=9)], 0) == -1                            # beyond 8:1 and 1:8 on the pass's axis
    assert call([row(1, wi=33, ss=33)], 1) == -1 and call([row(1, wi=1, wo=9)], 1) == -1
    assert call([row(0, sigma=1.0)], 0) == -1                                                                # noise on the height pass
    assert call([row(0)], 2) == -1 and call([row(0)], -1) == -1                                              # the axis
    assert call([row(0, wo=4)], 0) == -1 and call([row(1, ho=4)], 1) == -1                                   # the pass changes its own axis only
    torch.cuda.synchronize()
    assert bool((dst == 9).all())                                                                            # nothing ran
    assert call([row(0)], 0) == 0                                                                            # (the corrected call does run)
    torch.cuda.synchronize()
    mid = RT._round(RT.resize_axis0(img.astype(np.float64), 4, "bicubic"))
    assert torch.equal(dst[:96].cpu().view(4, 8, 3), torch.from_numpy(mid)) and bool((dst[96:] == 9).all())
    for kw in (dict(out_shapes=[(0, 8)]), dict(out_shapes=[(8, 65)]), dict(shapes=[(8, 0)]), dict(methods="lanczos"), dict(noise_sigma=[-1.0])):
        a = dict(offsets=[0], shapes=[(8, 8)], out_shapes=[(4, 4)], methods="bicubic")
        a.update(kw)
        with pytest.raises(_lib.PesrHipError):
            imresize_to_pool_u8(src.view(-1), **a)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_to_u8(src.cpu(), (4, 4))


# ---- the resize jitter in the sampler --------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(a.transpose(2, 0, 1).astype(np.float32))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_gpu_patch_sampler_with_resize_jitter(s):
    """assemble = [degrade restatement without noise -> resize restatement twice, the noise in the second -> JPEG restatement when on ->
    the crop / augment restatement], bit for bit; with jitter_hi = 0 the sampler returns what it returned before."""
    from data import augment
    from pesr_amd.degrade import DegradationSpec, kernel_size
    from pesr_amd.input_pipeline import GpuPatchSampler
    B, P = 6, 6
    hrs = [_rand(h, w, 700 + n) for n, (h, w) in enumerate(((11 * s + 1, 9 * s + s - 1), (8 * s, 13 * s)))]
    crops = [DO.modcrop(h, s) for h in hrs]
    for jpeg in ((0, 0), (30, 95)):
        spec = DegradationSpec(0.2 * s, 0.8 * s, True, 10.0, jpeg[0], jpeg[1], True, 0.125, 8.0)
        off = DegradationSpec(0.2 * s, 0.8 * s, True, 10.0, jpeg[0], jpeg[1], True)
        K = kernel_size(s, spec.sigma_hi)
        samp = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=spec)
        samp_off = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=off)
        rng = random.Random(5 + s)
        picks = [(b % 2, (b * 2) % (crops[b % 2].shape[0] // s - P + 1), (b * 3 + 1) % (crops[b % 2].shape[1] // s - P + 1), (5, 2, 7, 0, 3, 6)[b])
                 + spec.draw(rng) for b in range(B)]
        n_off = len(off.fields())
        assert all(len(p) == 4 + n_off + 3 for p in picks)
        lr, hr = samp.assemble(picks, P, nhwc=True)
        lr_off, hr_off = samp_off.assemble([p[:4 + n_off] for p in picks], P, nhwc=True)
        assert torch.equal(hr, hr_off) and lr.shape == (B, 3, P, P)
        for b, p in enumerate(picks):
            i, y, x, aug = p[:4]
            d = spec.named(p[4:])
            kern = DO.gaussian_kernel(K, d["sigma1"], d["sigma2"], d["theta"])
            hr_crop = crops[i][s * y:s * (y + P), s * x:s * (x + P)]
            clean = DO.degrade(crops[i], s, kern, 0.0, 0, (y, x, P, P))
            jit = RT.jitter(clean, d["jitter_r"], d["jitter_m1"], d["jitter_m2"], d["sigma_n"], d["q"])
            want = JO.jpeg(jit, d["jpeg_quality"], True) if jpeg[1] else jit
            l, h = augment(want, hr_crop, aug)
            assert torch.equal(lr[b].cpu(), _f32(l)), (s, jpeg, b, d)
            assert torch.equal(hr[b].cpu(), _f32(h)), (s, jpeg, b)
            # the same pick with the jitter off: noise in the degrade launch, as before
            noisy = DO.degrade(crops[i], s, kern, d["sigma_n"], d["q"], (y, x, P, P))
            l0, _ = augment(JO.jpeg(noisy, d["jpeg_quality"], True) if jpeg[1] else noisy, hr_crop, aug)
            assert torch.equal(lr_off[b].cpu(), _f32(l0)), (s, jpeg, b)
        # draw_for: the crop, the values drawn before, then r and the two filters, all from one stream
        a, c = random.Random(2), random.Random(2)
        for pick, i in zip(samp.draw_for([1, 0, 1], P, a), [1, 0, 1]):
            h, w, _ = samp.lr_shapes[i]
            assert pick == (i, c.randint(0, h - P), c.randint(0, w - P), c.randint(0, 7)) + off.draw(c) + (c.uniform(0.125, 8.0), c.randrange(3),
                                                                                                            c.randrange(3))
        assert a.getstate() == c.getstate()


def test_loader_with_resize_jitter_resumes_bit_identically():
    """r and the filters come from the GPU loader's stream, which the training state already holds (checkpoint.rng_snapshot): draw,
    save the loader state, draw on; restore, draw again - the same picks and the same patches."""
    import importlib.util
    from pesr_amd import checkpoint
    from pesr_amd.degrade import DegradationSpec
    from pesr_amd.input_pipeline import GpuPatchSampler
    spec_ = importlib.util.spec_from_file_location("entry_train_resize_jitter", os.path.join(ROOT, "train.py"))
    Tm = importlib.util.module_from_spec(spec_); spec_.loader.exec_module(Tm)
    hrs = [_rand(80 + 3 * n, 90 - 2 * n, 800 + n) for n in range(4)]
    samp = GpuPatchSampler.from_hr(hrs, DEV, scale=4, degradation=DegradationSpec(0.8, 3.2, False, 5.0, 20, 90, True, 0.3, 2.5))
    loader = Tm.GpuLoader(samp, 4, 16, len(hrs), 2, 0, 1)
    idx = loader.epoch_indices()

    def step(k):
        picks = samp.draw_for(idx[4 * k:4 * k + 4], 16, loader.rng, augment=True)
        return picks, samp.assemble(picks, 16, nhwc=True)

    step(0)
    snap = checkpoint.rng_snapshot(gpu_loader=loader)
    picks_a, (lr_a, hr_a) = step(1)
    other, _ = step(0)
    assert other != picks_a                                                   # the stream moved on
    checkpoint.rng_restore(snap, gpu_loader=loader)
    picks_b, (lr_b, hr_b) = step(1)
    assert picks_a == picks_b and len(picks_a[0]) == 13 and torch.equal(lr_a, lr_b) and torch.equal(hr_a, hr_b)


# ---- entry points, each in a fresh interpreter -------------------------------------------------------------------------------------
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
for tag, extra in {runs!r}:
    print("RUN_" + tag, flush=True)
    T.main({args!r} + ["--save_path", os.path.join({base!r}, tag)] + extra)
print("ENTRY_OK")
"""


def test_test_entrypoint_resize_jitter(tmp_path):
    """test.py --from_hr true --degradation classical --resize_jitter 0.37,bilinear,box at x2: the Generator sees the jittered LR image
    (noise in the second resize), the "bicubic" column is the upscale of that image; without the flag nothing changes."""
    import importlib.util
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    spec = importlib.util.spec_from_file_location("entry_test_resize_jitter", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    s = 2
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    hrs = {"a.png": _rand(24 * s + 1, 21 * s + 1, 4), "b.png": _rand(17 * s, 30 * s, 5)}
    for name, im in hrs.items():
        Image.fromarray(im).save(base / "HR" / name)
    torch.save(gen_sd_scaled(16, 1, s, seed=3), tmp_path / "g.pt")
    args = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "16", "--num_blocks", "1", "--scale", str(s),
            "--from_hr", "true", "--degradation", "classical", "--blur_sigma", "1.2", "--noise_sigma", "4", "--degrade_seed", "11"]
    runs = [("plain", []), ("jitter", ["--resize_jitter", "0.37,bilinear,box"]), ("both", ["--resize_jitter", "1.6", "--jpeg_quality", "40"])]
    r = subprocess.run([sys.executable, "-c", TEST_PROG.format(root=ROOT, args=args, runs=runs, base=str(tmp_path / "out"))], capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {m.group(1): m.group(2) for m in re.finditer(r"RUN_(\w+)\n(.*?)(?=RUN_|ENTRY_OK)", r.stdout, flags=re.S)}
    kern = DO.gaussian_kernel(8, 1.2)                                            # kernel_size(2, 1.2) = 8
    for i, (name, im) in enumerate(sorted(hrs.items())):
        hr = np.ascontiguousarray(RO.modcrop(im, s))
        q = 11 + i
        lr = {"plain": DO.degrade(hr, s, kern, 4.0, q),
              "jitter": RT.jitter(DO.degrade(hr, s, kern), 0.37, 1, 2, 4.0, q),
              "both": JO.jpeg(RT.jitter(DO.degrade(hr, s, kern), 1.6, 0, 0, 4.0, q), 40, True)}
        assert not np.array_equal(lr["plain"], lr["jitter"])
        for tag, extra in runs:
            m = re.search(re.escape(name) + r": PSNR-Y ([-\d.]+|inf) dB, bicubic ([-\d.]+|inf) dB", out[tag])
            assert m, out[tag]
            sr = np.asarray(Image.open(tmp_path / "out" / tag / "Toy" / name).convert("RGB"))
            want_sr, want_bic = _host_psnr_y(sr, hr), _host_psnr_y(RO.imresize(lr[tag], s, True), hr)
            assert abs(float(m.group(1)) - want_sr) <= 1e-9 and abs(float(m.group(2)) - want_bic) <= 1e-9, (tag, name)
            # the LR image handed to the Generator is the restatement's, bit for bit
            a = T.build_parser().parse_args(args + extra)
            lr_t, hr_t, bic_t = T.lr_from_hr(im, s, DEV, T.classical_kernel(a), a.noise_sigma, a.degrade_seed + i, T.jpeg_quality(a),
                                             a.jpeg_chroma == "420", T.resize_jitter(a))
            assert torch.equal(lr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(lr[tag])), (tag, name)
            assert torch.equal(bic_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(RO.imresize(lr[tag], s, True)))
            assert torch.equal(hr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(hr))


TRAIN_PROG = """
import importlib.util, os, random, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({root!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
random.seed(1); np.random.seed(1); torch.manual_seed(1)          # the Generator's initialisation
Tm.main(["--num_channels", "16", "--num_blocks", "1", "--patch_size", "16", "--batch_size", "4", "--max_iters", "2", "--phase", "pretrain",
         "--train_dataset", "Toy", "--valid_dataset", "Toy", "--num_repeats", "2", "--degradation", "classical", "--blur_aniso", "true",
         "--noise_sigma", "10", "--lr_from_hr", "true", "--gpu_pipeline", "true", "--num_epochs", "1", "--scale", "3",
         "--resize_jitter", "0.3,2.5", "--jpeg_quality", "30,95", "--check_point", {base!r}])
print("ENTRY_OK")
"""


def test_train_entrypoint_resize_jitter(tmp_path):
    """Two iterations of train.py --resize_jitter (with noise and JPEG) and its validation, in a fresh child process."""
    from PIL import Image
    rng = np.random.RandomState(8)
    for sub, szs in (("train", [(60, 67), (54, 57), (64, 60), (57, 72)]), ("valid", [(41, 47), (49, 44)])):
        d = tmp_path / "data" / "origin" / sub / "Toy" / "HR"
        d.mkdir(parents=True)
        for i, (h, w) in enumerate(szs):
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(d / f"{i}.png")
    r = subprocess.run([sys.executable, "-c", TRAIN_PROG.format(root=ROOT, base=str(tmp_path / "ck"))], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    out = r.stdout
    assert r.returncode == 0 and "ENTRY_OK" in out, out[-3000:] + r.stderr[-3000:]
    m = re.search(r"Epoch \[1/1\] lr \S+\s+l1 (\S+)", out)
    assert m and np.isfinite(float(m.group(1))) and float(m.group(1)) > 0, out[-2000:]
    m = re.search(r"Finish valid \[1/1\]\. PSNR: ([-\d.]+)dB", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    assert (tmp_path / "ck" / "pretrain" / "best_model.pt").exists()
