"""GPU: the JPEG round trip of docs/modes.md section 4l (pesr_amd/csrc/jpeg.hip through the C ABI) against the float64 restatement
of tests/jpeg_oracle.py - BIT FOR BIT, no excused pixels: the order of operations is fixed and nothing is fused, so kernel and
restatement perform the same IEEE operations - and its users: GpuPatchSampler.from_hr(degradation=spec with a JPEG range), the
loader's resume, test.py --jpeg_quality."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import degrade_oracle as DO
import jpeg_oracle as JO
import resize_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")

# around the 8 x 8 block and the 16 x 16 MCU; 15 x 17 has odd chroma sides, 48 x 48 is the training patch
SHAPES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33), (3, 40), (48, 48)]
QUALITIES = [1, 10, 49, 50, 75, 100]


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0), 40 + 3.5 * x + 1.5 * y, 220 - 2.0 * x - 2.5 * y + 20 * np.sin((x + y) / 3.0)], axis=2)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y + x) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _report(got, want, what):
    diff = got.astype(np.int32) - want.astype(np.int32)
    bad = np.argwhere(diff != 0)
    pytest.fail(f"{what}: {len(bad)} bytes differ (max {np.abs(diff).max()}), first at {bad[0].tolist()}")


def _check(img, q, c420, what):
    from pesr_amd.jpeg import jpeg_u8
    want = JO.jpeg(img, q, c420)
    got = jpeg_u8(torch.from_numpy(img).to(DEV), q, c420).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    if not torch.equal(got, torch.from_numpy(want)):
        _report(got.numpy(), want, f"{what} q={q} {'4:2:0' if c420 else '4:4:4'} {img.shape}")


@pytest.mark.parametrize("c420", [True, False])
def test_shapes_around_the_block_and_the_mcu_bit_exact(c420):
    for n, (h, w) in enumerate(SHAPES):
        for k in range(3):                                  # three of the six qualities per shape, all six over two shapes
            _check(_rand(h, w, 10 * n + k), QUALITIES[(3 * n + k) % 6], c420, "random")


@pytest.mark.parametrize("c420", [True, False])
def test_flat_checkerboard_and_smooth_bit_exact(c420):
    from pesr_amd.jpeg import jpeg_u8
    for q in QUALITIES:
        grey = np.full((19, 22, 3), 128, np.uint8)
        assert torch.equal(jpeg_u8(torch.from_numpy(grey).to(DEV), q, c420).cpu(), torch.from_numpy(grey))       # returns itself
    for v, q in ((200, 75), (77, 10), (131, 1), (255, 90), (0, 30)):
        _check(np.full((16, 24, 3), v, np.uint8), q, c420, f"flat {v}")
    for q in (10, 50, 100):
        _check(_checker(16, 16), q, c420, "checkerboard")
        _check(_checker(15, 17), q, c420, "checkerboard")
    out = jpeg_u8(torch.from_numpy(_checker(16, 16)).to(DEV), 50, c420)
    assert int(out.min()) == 0 and int(out.max()) == 255                       # the clamp after the inverse DCT was hit
    for q in (10, 49, 75, 100):
        _check(_smooth(48, 48), q, c420, "smooth")
        _check(_smooth(37, 53), q, c420, "smooth")


def _pool_case():
    """Ten windows inside three bigger images laid out with odd gaps: (image, y0, x0, h, w, q)."""
    imgs = [_rand(40, 50, 501), _smooth(33, 47), _rand(20, 64, 502)]
    offs, flat, pos = [], [], 0
    for n, im in enumerate(imgs):
        gap = [1, 2, 5][n]
        flat.append(np.full(gap, 77, np.uint8)); pos += gap
        offs.append(pos); flat.append(im.reshape(-1)); pos += im.size
    wins = [(0, 0, 0, 16, 16, 75), (0, 0, 16, 15, 17, 10), (0, 17, 1, 23, 15, 1), (0, 16, 33, 24, 17, 100), (0, 39, 16, 1, 1, 50),
            (1, 0, 0, 33, 20, 49), (1, 0, 21, 7, 9, 90), (1, 8, 20, 25, 27, 30), (2, 0, 0, 20, 64, 60), (0, 16, 16, 1, 17, 85)]
    return imgs, offs, np.concatenate(flat), wins


@pytest.mark.parametrize("c420", [True, False])
def test_one_call_many_windows_then_in_place(c420):
    from pesr_amd.jpeg import jpeg_pool_u8
    imgs, offs, flat, wins = _pool_case()
    # the windows do not overlap
    cover = [np.zeros(im.shape[:2], np.int32) for im in imgs]
    for i, y0, x0, h, w, _ in wins:
        cover[i][y0:y0 + h, x0:x0 + w] += 1
    assert all(c.max() == 1 for c in cover)
    widths = [im.shape[1] for im in imgs]
    o = [offs[i] + 3 * (y0 * widths[i] + x0) for i, y0, x0, _, _, _ in wins]
    assert any(v % 4 for v in o) and len({q for *_, q in wins}) == len(wins)
    pool = torch.from_numpy(flat).to(DEV)
    out, ooffs = jpeg_pool_u8(pool, o, [(h, w) for _, _, _, h, w, _ in wins], [widths[i] for i, *_ in wins], [q for *_, q in wins], c420)
    assert torch.equal(pool.cpu(), torch.from_numpy(flat))                     # the source is not touched
    assert out.dtype == torch.uint8 and out.numel() == sum(3 * h * w for _, _, _, h, w, _ in wins)
    want_pool = flat.copy()
    for e, (i, y0, x0, h, w, q) in enumerate(wins):
        want = JO.jpeg_window(flat, o[e], widths[i], h, w, q, c420)
        assert np.array_equal(want, JO.jpeg(imgs[i][y0:y0 + h, x0:x0 + w], q, c420))
        got = out[ooffs[e]:ooffs[e] + 3 * h * w].view(h, w, 3).cpu()
        if not torch.equal(got, torch.from_numpy(want)):
            _report(got.numpy(), want, f"window {e} {(i, y0, x0, h, w, q)}")
        for y in range(h):
            want_pool[o[e] + 3 * widths[i] * y:o[e] + 3 * widths[i] * y + 3 * w] = want[y].reshape(-1)
    # the same call in place: every window replaced where it lies, every other byte as it was
    same, soffs = jpeg_pool_u8(pool, o, [(h, w) for _, _, _, h, w, _ in wins], [widths[i] for i, *_ in wins], [q for *_, q in wins], c420, out=pool)
    assert same is pool and soffs == o
    if not torch.equal(pool.cpu(), torch.from_numpy(want_pool)):
        _report(pool.cpu().numpy(), want_pool, "in place")


def test_invalid_arguments_return_einval_and_launch_nothing():
    from pesr_amd import _lib
    from pesr_amd.jpeg import _device_tables, jpeg_pool_u8, jpeg_u8
    L = _lib.lib()
    img = _rand(12, 20, 1)
    src = torch.from_numpy(img).to(DEV)
    dst = torch.full((4096,), 9, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    T, quant = _device_tables(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rows, chroma=420, n=None, ws_bytes=4096):
        d = np.array(rows, dtype=np.int64).reshape(-1, 8)
        dd = torch.from_numpy(d).to(DEV)
        return L.pesr_jpeg_u8(src.data_ptr(), dst.data_ptr(), d.ctypes.data_as(ctypes.c_void_p), dd.data_ptr(), len(d) if n is None else n, chroma,
                              T.data_ptr(), quant.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    def row(so=0, ss=20, do=0, ds=20, h=12, w=20, q=75, wo=0):
        return (so, ss, do, ds, h, w, q, wo)

    assert call([row(q=0)]) == -1 and call([row(q=101)]) == -1 and call([row(q=-5)]) == -1          # q outside 1 .. 100
    assert call([row(h=0)]) == -1 and call([row(w=0)]) == -1 and call([row(h=-3)]) == -1            # h or w < 1
    assert call([row(ss=19)]) == -1 and call([row(ds=19)]) == -1                                    # stride < w
    assert call([row()], n=0) == -1 and call([row()], n=-1) == -1                                   # n < 1
    need = 12 * 20 + 2 * 6 * 10
    assert call([row()], ws_bytes=need - 1) == -1 and call([row()], chroma=444, ws_bytes=3 * 12 * 20 - 1) == -1   # workspace too small
    assert call([row()], chroma=422) == -1 and call([row()], chroma=0) == -1 and call([row()], chroma=1) == -1    # chroma mode
    assert call([row(so=-1)]) == -1 and call([row(do=-1)]) == -1 and call([row(wo=4)]) == -1
    assert call([row(h=6), row(h=0, so=360, do=360, wo=6 * 20 + 2 * 3 * 10)]) == -1                  # an invalid entry among valid ones
    torch.cuda.synchronize()
    assert bool((dst == 9).all()) and bool((ws == 0).all())                                         # nothing ran
    assert call([row()], ws_bytes=need) == 0                                                        # (the corrected call does run)
    torch.cuda.synchronize()
    assert torch.equal(dst[:720].cpu().view(12, 20, 3), torch.from_numpy(JO.jpeg(img, 75))) and bool((dst[720:] == 9).all())
    for kw in (dict(shapes=[(0, 20)]), dict(strides=[19]), dict(qualities=[0]), dict(qualities=[101])):
        a = dict(offsets=[0], shapes=[(12, 20)], strides=[20], qualities=[50])
        a.update(kw)
        with pytest.raises(_lib.PesrHipError):
            jpeg_pool_u8(src.view(-1), **a)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        jpeg_u8(src.cpu(), 50)


@pytest.mark.parametrize("s", [2, 4])
def test_gpu_patch_sampler_with_jpeg(s):
    """assemble = [degrade restatement -> JPEG restatement -> the crop / augment restatement], bit for bit; the block grid starts at
    the patch's origin and the compression precedes the flips / transpose."""
    from data import augment
    from pesr_amd.degrade import DegradationSpec, kernel_size
    from pesr_amd.input_pipeline import GpuPatchSampler
    B, P = 4, 16
    hrs = [_rand(h, w, 700 + n) for n, (h, w) in enumerate(((21 * s + 1, 19 * s + s - 1), (18 * s, 25 * s)))]
    crops = [DO.modcrop(h, s) for h in hrs]
    for c420 in (True, False):
        spec = DegradationSpec(0.2 * s, 0.8 * s, True, 10.0, 30, 95, c420)
        off = DegradationSpec(0.2 * s, 0.8 * s, True, 10.0)
        K = kernel_size(s, spec.sigma_hi)
        samp = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=spec)
        samp_off = GpuPatchSampler.from_hr(hrs, DEV, scale=s, degradation=off)
        rng = random.Random(5)
        picks = [(b % 2, (b * 2) % (crops[b % 2].shape[0] // s - P + 1), (b * 3 + 1) % (crops[b % 2].shape[1] // s - P + 1), (5, 2, 7, 0)[b]) + spec.draw(rng)
                 for b in range(B)]
        assert all(len(p) == 10 and 30 <= p[9] <= 95 for p in picks)
        for nhwc in (False, True):
            lr, hr = samp.assemble(picks, P, nhwc=nhwc)
            lr_off, hr_off = samp_off.assemble([p[:9] for p in picks], P, nhwc=nhwc)
            assert torch.equal(hr, hr_off) and lr.shape == (B, 3, P, P)
            for b, (i, y, x, aug, s1, s2, th, sn, q, quality) in enumerate(picks):
                win = DO.degrade(crops[i], s, DO.gaussian_kernel(K, s1, s2, th), sn, q, (y, x, P, P))
                hr_crop = crops[i][s * y:s * (y + P), s * x:s * (x + P)]
                l, h = augment(JO.jpeg(win, quality, c420), hr_crop, aug)
                assert torch.equal(lr[b].cpu(), torch.from_numpy(l.transpose(2, 0, 1).astype(np.float32))), (c420, nhwc, b)
                assert torch.equal(hr[b].cpu(), torch.from_numpy(h.transpose(2, 0, 1).astype(np.float32))), (c420, nhwc, b)
                # the same pick with JPEG off: what it was before
                l0, _ = augment(win, hr_crop, aug)
                assert torch.equal(lr_off[b].cpu(), torch.from_numpy(l0.transpose(2, 0, 1).astype(np.float32))), (c420, nhwc, b)
        # draw_for: the crop, the spec's five values, then the quality, all from one stream
        a, b = random.Random(2), random.Random(2)
        for pick, i in zip(samp.draw_for([1, 0, 1], P, a), [1, 0, 1]):
            h, w, _ = samp.lr_shapes[i]
            assert pick == (i, b.randint(0, h - P), b.randint(0, w - P), b.randint(0, 7)) + off.draw(b) + (b.randint(30, 95),)
        assert a.getstate() == b.getstate()


def test_loader_with_jpeg_resumes_bit_identically():
    """The quality comes from the GPU loader's stream, which the training state already holds (checkpoint.rng_snapshot): draw, save
    the loader state, draw on; restore, draw again - the same picks and the same patches."""
    import importlib.util
    from pesr_amd import checkpoint
    from pesr_amd.degrade import DegradationSpec
    from pesr_amd.input_pipeline import GpuPatchSampler
    spec_ = importlib.util.spec_from_file_location("entry_train_jpeg", os.path.join(ROOT, "train.py"))
    Tm = importlib.util.module_from_spec(spec_); spec_.loader.exec_module(Tm)
    hrs = [_rand(80 + 3 * n, 90 - 2 * n, 800 + n) for n in range(4)]
    samp = GpuPatchSampler.from_hr(hrs, DEV, scale=4, degradation=DegradationSpec(0.8, 3.2, False, 5.0, 20, 90))
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
    assert picks_a == picks_b and len(picks_a[0]) == 10 and torch.equal(lr_a, lr_b) and torch.equal(hr_a, hr_b)


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


def test_test_entrypoint_jpeg_quality(tmp_path):
    """test.py --from_hr true --jpeg_quality 30 at x2: the Generator sees the compressed LR image, the "bicubic" column is the upscale
    of the compressed image; without the flag nothing changes (the PNGs of two runs without it, one naming only --jpeg_chroma, are
    the same bytes, and its columns are those of the uncompressed LR image)."""
    import importlib.util
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    spec = importlib.util.spec_from_file_location("entry_test_jpeg", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    s = 2
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    hrs = {"a.png": _smooth(24 * s + 1, 21 * s + 1), "b.png": _rand(17 * s, 30 * s, 5)}
    for name, im in hrs.items():
        Image.fromarray(im).save(base / "HR" / name)
    torch.save(gen_sd_scaled(16, 1, s, seed=3), tmp_path / "g.pt")
    args = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "16", "--num_blocks", "1", "--scale", str(s),
            "--from_hr", "true"]
    runs = [("plain", []), ("chroma_only", ["--jpeg_chroma", "444"]), ("jpeg", ["--jpeg_quality", "30"])]
    r = subprocess.run([sys.executable, "-c", TEST_PROG.format(root=ROOT, args=args, runs=runs, base=str(tmp_path / "out"))], capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {m.group(1): m.group(2) for m in re.finditer(r"RUN_(\w+)\n(.*?)(?=RUN_|ENTRY_OK)", r.stdout, flags=re.S)}
    for name, im in hrs.items():
        hr = RO.modcrop(im, s)
        lr_plain = RO.imresize(hr, s, False)
        lr_jpeg = JO.jpeg(lr_plain, 30, True)
        assert not np.array_equal(lr_plain, lr_jpeg)
        png = {tag: (tmp_path / "out" / tag / "Toy" / name).read_bytes() for tag, _ in runs}
        assert png["plain"] == png["chroma_only"] and png["plain"] != png["jpeg"]
        for tag, lr in (("plain", lr_plain), ("chroma_only", lr_plain), ("jpeg", lr_jpeg)):
            m = re.search(re.escape(name) + r": PSNR-Y ([-\d.]+|inf) dB, bicubic ([-\d.]+|inf) dB", out[tag])
            assert m, out[tag]
            sr = np.asarray(Image.open(tmp_path / "out" / tag / "Toy" / name).convert("RGB"))
            want_sr, want_bic = _host_psnr_y(sr, hr), _host_psnr_y(RO.imresize(lr, s, True), hr)
            assert abs(float(m.group(1)) - want_sr) <= 1e-9 and abs(float(m.group(2)) - want_bic) <= 1e-9, (tag, name)
        # the LR image fed to the model is the restatement's, bit for bit; without a quality it is the bicubic one, as before
        a = T.build_parser().parse_args(args + ["--jpeg_quality", "30"])
        lr_t, hr_t, bic_t = T.lr_from_hr(im, s, DEV, None, 0.0, 0, T.jpeg_quality(a), a.jpeg_chroma == "420")
        assert torch.equal(lr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(lr_jpeg))
        assert torch.equal(bic_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(RO.imresize(lr_jpeg, s, True)))
        assert torch.equal(hr_t[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(np.ascontiguousarray(hr)))
        lr_0, _, _ = T.lr_from_hr(im, s, DEV)
        assert torch.equal(lr_0[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(lr_plain))
        # classical degradation, then 4:4:4 compression
        lr_c, _, _ = T.lr_from_hr(im, s, DEV, np.full((2, 2), 0.25), 4.0, 3, 60, False)
        assert torch.equal(lr_c[0].permute(1, 2, 0).to(torch.uint8).cpu(), torch.from_numpy(JO.jpeg(DO.degrade(hr, s, np.full((2, 2), 0.25), 4.0, 3), 60, False)))
