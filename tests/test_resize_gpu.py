"""GPU: the bicubic resize of docs/modes.md section 4f (pesr_amd/csrc/resize.hip through the C ABI) against the float64
restatement of tests/resize_oracle.py - BIT FOR BIT, no excused pixels: the order of operations is fixed and nothing is fused, so
kernel and restatement perform the same IEEE operations - and its users: GpuPatchSampler.from_hr, test.py --from_hr,
train.py --lr_from_hr."""
import ctypes
import importlib.util
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (5 * x + 2 * y) // 2 % 256], axis=2).astype(np.uint8)


def _check(img, s, up, what):
    from pesr_amd.resize import imresize_u8
    want = RO.imresize(img, s, up)
    got = imresize_u8(torch.from_numpy(img).to(DEV), s, up).cpu()
    if not torch.equal(got, torch.from_numpy(want)):
        diff = (got.numpy().astype(np.int32) - want.astype(np.int32))
        bad = np.argwhere(diff != 0)
        near = RO.near_ties(img, s, up) if s == 3 else "n/a"
        # a mismatch with near-ties > 0 points at a contracted multiply-add, one with 0 at indexing
        pytest.fail(f"{what} x{s} {'up' if up else 'down'} {img.shape}: {len(bad)} bytes differ (max {np.abs(diff).max()}), first at "
                    f"{bad[0].tolist()}; restatement values within 1e-9 of a tie without being one: {near}")


# LR-side sizes (h, w): the down-resize takes the s-fold image, the up-resize this one.  3w % 4 = 1, 2, 3 (row tails and misaligned
# row starts); one output pixel (every tap reflected); 2s; above one workgroup's tile along a row (340 pixels / 1024 bytes)
SIZES = [(1, 1), (2, 2), (5, 7), (6, 10), (9, 13), (3, 345), (40, 2)]


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_imresize_bit_exact_edge_sizes(s, up):
    for n, (h, w) in enumerate(SIZES):
        k = 1 if up else s
        _check(_rand(k * h, k * w, 100 + n), s, up, "random")


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_imresize_bit_exact_ramp_and_clamp(s, up):
    k = 1 if up else s
    _check(_ramp(k * 24, k * 31), s, up, "ramp")                     # the tie-heavy case at x2 / x4
    _check(np.zeros((k * 6, k * 5, 3), np.uint8), s, up, "all-0")
    _check(np.full((k * 6, k * 5, 3), 255, np.uint8), s, up, "all-255")
    # black / white blocks: the cubic's overshoot leaves [0, 255] on both sides
    img = np.zeros((k * 12, k * 12, 3), np.uint8)
    img[k * 3:k * 8, k * 4:k * 9] = 255
    _check(img, s, up, "blocks")


@pytest.mark.parametrize("s", [2, 3, 4])
def test_imresize_bit_exact_2k_image(s):
    img = _rand(1356, 2040, 7)
    _check(RO.modcrop(img, s), s, False, "2040x1356")
    _check(RO.imresize(RO.modcrop(img, s), s, False), s, True, "2040x1356 LR")


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_pool_form_equals_per_image_calls(s, up):
    from pesr_amd.resize import imresize_pool_u8, imresize_u8
    k = 1 if up else s
    imgs = [_rand(k * h, k * w, 200 + n) for n, (h, w) in enumerate([(5, 7), (1, 1), (8, 3), (3, 345)])]
    # images back to back with odd gaps: offsets that are not multiples of 4
    offs, flat, pos = [], [], 0
    for n, im in enumerate(imgs):
        gap = [1, 2, 3, 5][n]
        flat.append(np.full(gap, 77, np.uint8)); pos += gap
        offs.append(pos); flat.append(im.reshape(-1)); pos += im.size
    assert any(o % 4 for o in offs)
    pool = torch.from_numpy(np.concatenate(flat)).to(DEV)
    out, ooffs, oshapes = imresize_pool_u8(pool, offs, [im.shape[:2] for im in imgs], s, up)
    assert out.dtype == torch.uint8 and out.dim() == 1
    for im, o, (h, w) in zip(imgs, ooffs, oshapes):
        one = imresize_u8(torch.from_numpy(im).to(DEV), s, up)
        assert one.shape == (h, w, 3)
        assert torch.equal(out[o:o + 3 * h * w].view(h, w, 3), one)
        assert torch.equal(one.cpu(), torch.from_numpy(RO.imresize(im, s, up)))
    assert ooffs[-1] + 3 * oshapes[-1][0] * oshapes[-1][1] == out.numel()


def test_invalid_arguments_return_einval_and_launch_nothing():
    from pesr_amd import _lib
    from pesr_amd.resize import imresize_u8, resize_weights
    L = _lib.lib()
    src = torch.from_numpy(_rand(8, 10, 1)).to(DEV)
    dst = torch.full((8 * 10 * 3 * 16,), 9, dtype=torch.uint8, device=DEV)
    wts = np.zeros(16); wts[:8] = resize_weights(2, False)
    stream = torch.cuda.current_stream().cuda_stream

    def call(desc_rows, axis, s, up):
        d = np.array(desc_rows, dtype=np.int64)
        dd = torch.from_numpy(d).to(DEV)
        return L.pesr_imresize_u8_pass(src.data_ptr(), dst.data_ptr(), d.ctypes.data_as(ctypes.c_void_p), dd.data_ptr(), len(d), axis, s, up,
                                       wts.ctypes.data_as(ctypes.c_void_p), stream)

    assert call([(0, 0, 8, 10)], 0, 5, 0) == -1                  # s outside {2, 3, 4}
    assert call([(0, 0, 8, 10)], 0, 1, 1) == -1
    assert call([(0, 0, 8, 10)], 0, 3, 0) == -1                  # 8 rows do not divide by 3
    assert call([(0, 0, 8, 10)], 1, 4, 0) == -1                  # 10 columns do not divide by 4
    assert call([(0, 0, 8, 10), (0, 120, 0, 10)], 0, 2, 0) == -1  # an empty image among valid ones
    assert call([(0, 0, 8, 10)], 2, 2, 0) == -1                  # no such axis
    torch.cuda.synchronize()
    assert bool((dst == 9).all())                                # nothing ran
    assert call([(0, 0, 8, 10)], 0, 2, 0) == 0                   # (the same call with valid arguments does run)
    torch.cuda.synchronize()
    assert not bool((dst[:4 * 10 * 3] == 9).all()) and bool((dst[4 * 10 * 3:] == 9).all())
    for s, img in ((5, src), (3, src), (4, src)):
        with pytest.raises(_lib.PesrHipError):
            imresize_u8(img, s, False)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        imresize_u8(src.cpu(), 2, False)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_gpu_patch_sampler_from_hr_bit_exact(s):
    from data import augment
    from pesr_amd.input_pipeline import GpuPatchSampler
    hrs = [_rand(h, w, 300 + n) for n, (h, w) in enumerate(((11 * s + 1, 9 * s + s - 1), (8 * s, 13 * s), (9 * s + 1, 8 * s)))]
    crops = [RO.modcrop(h, s) for h in hrs]
    lrs = [RO.imresize(c, s, False) for c in crops]
    samp = GpuPatchSampler.from_hr(hrs, DEV, scale=s)
    old = GpuPatchSampler(lrs, crops, DEV, scale=s)                      # the existing constructor, fed the restatement's LR
    assert samp.n == 3 and samp.scale == s and [tuple(x) for x in samp.lr_shapes] == [l.shape for l in lrs]
    assert torch.equal(samp.lr_pool, old.lr_pool) and torch.equal(samp.hr_pool, old.hr_pool)
    assert list(samp.lr_off) == list(old.lr_off) and list(samp.hr_off) == list(old.hr_off)
    P = 6
    picks = [(b % 3, (b * 2) % (lrs[b % 3].shape[0] - P + 1), (b * 3) % (lrs[b % 3].shape[1] - P + 1), b % 8) for b in range(16)]
    assert {p[3] for p in picks} == set(range(8))                        # all 8 augmentations
    for nhwc in (False, True):
        lr, hr = samp.assemble(picks, P, nhwc=nhwc)
        lr_old, hr_old = old.assemble(picks, P, nhwc=nhwc)
        assert torch.equal(lr, lr_old) and torch.equal(hr, hr_old)
        for b, (i, y, x, aug) in enumerate(picks):
            l, h = augment(lrs[i][y:y + P, x:x + P], crops[i][s * y:s * (y + P), s * x:s * (x + P)], aug)
            assert torch.equal(lr[b].cpu(), torch.from_numpy(l.transpose(2, 0, 1).astype(np.float32)))
            assert torch.equal(hr[b].cpu(), torch.from_numpy(h.transpose(2, 0, 1).astype(np.float32)))
    rnd = samp.draw(5, P, random.Random(2))
    assert all(0 <= y <= lrs[i].shape[0] - P and 0 <= x <= lrs[i].shape[1] - P for i, y, x, _ in rnd)


def _host_psnr_y(a, b):
    """utils.compute_PSNR's host formula on two uint8 HWC arrays."""
    coef = np.array([65.738, 129.057, 25.064]) / 256.0
    ya = np.clip(np.dot(a.astype(np.float64), coef) + 16, 0, 255).round()
    yb = np.clip(np.dot(b.astype(np.float64), coef) + 16, 0, 255).round()
    return 20 * np.log10(255 / np.sqrt(np.mean((ya - yb) ** 2)))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_test_entrypoint_from_hr(tmp_path, monkeypatch, capsys, s):
    """test.py --from_hr true on an HR-only folder (a 16-channel, 1-block seeded Generator: the narrowest the HIP convs take)."""
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    spec = importlib.util.spec_from_file_location(f"entry_test_from_hr{s}", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    hrs = {"a.png": _ramp(12 * s + 1, 10 * s + s - 1), "b.png": _rand(9 * s, 14 * s, 5)}
    for name, im in hrs.items():
        Image.fromarray(im).save(base / "HR" / name)
    torch.save(gen_sd_scaled(16, 1, s, seed=3), tmp_path / "g.pt")
    common = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "16", "--num_blocks", "1", "--scale", str(s)]
    T.main(common + ["--from_hr", "true", "--save_path", str(tmp_path / "out")])
    text = capsys.readouterr().out
    seen = []
    for name, im in hrs.items():
        hr = RO.modcrop(im, s)
        sr = np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB"))
        assert sr.shape == hr.shape                                       # PNGs at (mod-cropped) HR size
        m = re.search(re.escape(name) + r": PSNR-Y ([-\d.]+|inf) dB, bicubic ([-\d.]+|inf) dB", text)
        assert m, text
        bic = RO.imresize(RO.imresize(hr, s, False), s, True)
        want_sr, want_bic = _host_psnr_y(sr, hr), _host_psnr_y(bic, hr)
        print(f"x{s} {name}: printed {m.group(1)} / {m.group(2)}, host formula {want_sr!r} / {want_bic!r}")
        assert abs(float(m.group(1)) - want_sr) <= 1e-9 and abs(float(m.group(2)) - want_bic) <= 1e-9       # (10 decimals are printed)
        # the pieces behind the printed line: the device LR and bicubic images are the restatement's, bit for bit
        from utils import compute_PSNR
        lr_t, hr_t, bic_t = T.lr_from_hr(im, s, DEV)
        assert torch.equal(bic_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(bic))
        assert torch.equal(lr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(RO.imresize(hr, s, False)))
        assert abs(compute_PSNR(bic_t, hr_t) - want_bic) <= 1e-9
        seen.append((want_sr, want_bic))
    m = re.search(r"Mean PSNR-Y ([-\d.]+) dB, bicubic ([-\d.]+) dB", text)
    assert m and abs(float(m.group(1)) - np.mean([p[0] for p in seen])) <= 1e-9 and abs(float(m.group(2)) - np.mean([p[1] for p in seen])) <= 1e-9
    # without the flag: LR/ is read, nothing but the usual lines is printed, and the PNG is the model's output for THAT LR image
    (base / "LR").mkdir()
    lr_img = _rand(7, 9, 11)
    Image.fromarray(lr_img).save(base / "LR" / "c.png")
    capsys.readouterr()
    T.main(common + ["--save_path", str(tmp_path / "out2")])
    text = capsys.readouterr().out
    assert [l for l in text.splitlines() if not l.startswith("Number of parameters")] == ["Tested 1 img(s)", "Finish"]
    assert os.listdir(tmp_path / "out2" / "Toy") == ["c.png"]
    assert np.asarray(Image.open(tmp_path / "out2" / "Toy" / "c.png")).shape == (7 * s, 9 * s, 3)


@pytest.mark.parametrize("pipeline", ["host", "gpu"])
def test_train_entrypoint_lr_from_hr(tmp_path, pipeline):
    """train.py --phase pretrain --lr_from_hr true --max_iters 2 on HR-only folders, host loader and --gpu_pipeline true, each in a
    fresh interpreter with its own time limit."""
    from PIL import Image
    rng = np.random.RandomState(8)
    for sub, sizes in (("train", [(60, 67), (54, 57), (64, 60), (57, 72)]), ("valid", [(25, 31)])):
        d = tmp_path / "data" / "origin" / sub / "Toy" / "HR"
        d.mkdir(parents=True)
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(d / f"{i}.png")
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
Tm.main(["--scale", "3", "--num_channels", "16", "--num_blocks", "1", "--patch_size", "16", "--batch_size", "4", "--num_epochs", "1",
         "--max_iters", "2", "--check_point", {ck!r}, "--train_dataset", "Toy", "--valid_dataset", "Toy", "--num_repeats", "2",
         "--phase", "pretrain", "--lr_from_hr", "true", "--gpu_pipeline", {"true" if pipeline == "gpu" else "false"!r}])
print("ENTRY_OK")
"""
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"Epoch \[1/1\] lr \S+\s+l1 (\S+)", r.stdout)
    assert m and np.isfinite(float(m.group(1))) and float(m.group(1)) > 0, r.stdout[-2000:]
    m = re.search(r"Finish valid \[1/1\]\. PSNR: ([-\d.]+)dB", r.stdout)
    assert m and np.isfinite(float(m.group(1))), r.stdout[-2000:]
    assert (tmp_path / "ck" / "pretrain" / "best_model.pt").exists()
