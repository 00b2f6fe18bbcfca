"""GPU: SSIM-Y with a border shave (pesr_amd/csrc/ssim.hip through the C ABI, docs/modes.md section 4g) against the float64
restatement of tests/ssim_oracle.py.  The MAP is compared BIT FOR BIT: the order of operations is fixed and nothing is fused, so
kernel and restatement perform the same IEEE operations.  The MEAN is held to the worst case of summing n values of magnitude <= 1
in any order, (n - 1) * 2^-53, against the exactly summed map.  Then its users: utils.compute_SSIM, test.py --ssim / --shave,
train.py --valid_ssim."""
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_oracle as RO
import ssim_oracle as SO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _images(kind, n, h, w, seed):
    """Two [n, 3, h, w] float32 arrays.  u8: a blocky uint8-valued image and a noisy copy.  float: the second one is what a
    Generator puts out: non-integer values in about -20 .. 280."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, 3, (h + 7) // 8, (w + 7) // 8)).astype(np.float64)
    a = np.kron(base, np.ones((8, 8)))[:, :, :h, :w]
    b = a + rng.normal(0.0, 8.0, a.shape)
    if kind == "u8":
        b = np.clip(np.rint(b), 0, 255)
    else:
        b = b * (300.0 / 255.0) - 20.0 + rng.uniform(-0.5, 0.5, a.shape)
    return a.astype(np.float32), b.astype(np.float32)


def _to_dev(x, layout):
    t = torch.from_numpy(x).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if layout == "l" else t.contiguous()


# (H, W, N, shave, layouts of a and b: c = NCHW-contiguous, l = channels_last, values)
# 11 x 11 is one output pixel; 12 x 43, 97 x 131 and 1356 x 2040 are no multiples of any tile in either direction
CASES = [
    (11, 11, 1, 0, "cc", "u8"),
    (11, 11, 3, 0, "ll", "float"),
    (19, 21, 1, 4, "lc", "u8"),
    (12, 43, 1, 0, "cl", "u8"),
    (43, 12, 3, 0, "lc", "float"),
    (97, 131, 1, 0, "cc", "u8"),
    (97, 131, 1, 2, "ll", "float"),
    (97, 131, 3, 4, "lc", "float"),
    (131, 97, 1, 4, "cl", "u8"),
    (256, 256, 1, 0, "ll", "u8"),
    (256, 256, 3, 2, "cc", "float"),
    (256, 256, 1, 4, "cl", "float"),
    (1356, 2040, 1, 0, "cc", "u8"),
    (1356, 2040, 1, 4, "cl", "float"),
]


@pytest.mark.parametrize("h,w,n,shave,layouts,kind", CASES)
def test_map_bit_for_bit_and_mean(h, w, n, shave, layouts, kind):
    from pesr_amd import ops
    a, b = _images(kind, n, h, w, seed=1000 + h + 7 * w + n + shave)
    ta, tb = _to_dev(a, layouts[0]), _to_dev(b, layouts[1])
    got, gmap = ops.ssim_y(ta, tb, shave, return_map=True)
    assert got.dtype == gmap.dtype == torch.float64 and got.shape == (n,)
    assert gmap.shape == (n, h - 2 * shave - 10, w - 2 * shave - 10)
    again, gmap2 = ops.ssim_y(ta, tb, shave, return_map=True)
    plain = ops.ssim_y(ta, tb, shave)
    assert torch.equal(again, got) and torch.equal(gmap2, gmap)          # deterministic: the same bits on every call
    assert torch.equal(plain, got)                                        # and with or without the map
    got, gmap = got.cpu().numpy(), gmap.cpu().numpy()
    for i in range(n):
        want = SO.ssim_map(a[i], b[i], shave)
        if not np.array_equal(gmap[i], want):
            bad = np.argwhere(gmap[i] != want)
            pytest.fail(f"image {i}: {len(bad)} of {want.size} map elements differ, first at {bad[0].tolist()}: "
                        f"{gmap[i][tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}, max |diff| {np.max(np.abs(gmap[i] - want)):.3e}")
        cnt = want.size
        mean = math.fsum(want.ravel().tolist()) / cnt
        diff = abs(float(got[i]) - mean)
        print(f"{h} x {w} shave {shave} image {i}: ssim {float(got[i])!r}, fsum(map)/n {mean!r}, |diff| {diff:.3e}, "
              f"bound {(cnt - 1) * 2.0 ** -53:.3e}")
        assert diff <= (cnt - 1) * 2.0 ** -53
    if kind == "u8" and n == 1:
        one = ops.ssim_y(ta, ta, shave, return_map=True)
        assert float(one[0][0]) == 1.0 and bool((one[1] == 1.0).all())   # an image against itself: exactly 1 everywhere


def test_non_contiguous_views_and_refusals():
    from pesr_amd import _lib, ops
    a, b = _images("float", 2, 40, 52, seed=5)
    big_a, big_b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    va, vb = big_a[:, :, 3:37, 5:50], big_b[:, :, 3:37, 5:50]            # neither layout: ops makes them contiguous
    got, gmap = ops.ssim_y(va, vb, 1, return_map=True)
    for i in range(2):
        assert np.array_equal(gmap[i].cpu().numpy(), SO.ssim_map(a[i, :, 3:37, 5:50], b[i, :, 3:37, 5:50], 1))
    with pytest.raises(ValueError):
        ops.ssim_y(big_a, big_b, 15)                                      # 10 x 22 left
    with pytest.raises(ValueError):
        ops.ssim_y(big_a[..., :10], big_b[..., :10])
    with pytest.raises(ValueError):
        ops.ssim_y(big_a, big_b[..., :51])
    with pytest.raises(ValueError):
        ops.ssim_y(big_a, big_b, -1)
    with pytest.raises(_lib.PesrHipError):
        ops.ssim_y(big_a.double(), big_b.double())
    with pytest.raises(_lib.PesrHipError):
        ops.ssim_y(big_a.cpu(), big_b.cpu())


def test_compute_ssim_device_path_and_untouched_margins(monkeypatch):
    import utils
    from pesr_amd import _lib, ops
    n, h, w, shave = 2, 45, 70, 2
    a, b = _images("float", n, h, w, seed=9)
    # utils.compute_SSIM on GPU tensors is ops.ssim_y (the mean over the pairs; one pair: that pair's value)
    ta, tb = _to_dev(a, "c"), _to_dev(b, "l")
    calls = []
    real = ops.ssim_y
    monkeypatch.setattr(ops, "ssim_y", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    one = utils.compute_SSIM(ta[:1], tb[:1], shave)
    both = utils.compute_SSIM(ta, tb, shave)
    monkeypatch.undo()
    assert len(calls) == 2
    dev = ops.ssim_y(ta, tb, shave)
    assert one == float(dev[0]) and both == float(dev.mean())
    assert one == float(ops.ssim_y(ta[:1], tb[:1].contiguous(), shave)[0])
    host = utils.compute_SSIM(ta[:1].cpu(), tb[:1].cpu(), shave)
    assert abs(host - one) <= 1e-12
    # margins: inputs surrounded by NaN (a read outside would poison the map), outputs and workspace surrounded by a sentinel
    M = 4096
    ho, wo = h - 2 * shave - 10, w - 2 * shave - 10
    ins = []
    for x in (a, b):
        flat = torch.full((x.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
        flat[M:M + x.size] = torch.from_numpy(x).to(DEV).reshape(-1)
        ins.append(flat)
    sentinel = -12345.678
    out = torch.full((n + 2 * M,), sentinel, dtype=torch.float64, device=DEV)
    smap = torch.full((n * ho * wo + 2 * M,), sentinel, dtype=torch.float64, device=DEV)
    ws_doubles = n * ((ho + 15) // 16) * ((wo + 15) // 16)
    ws = torch.full((ws_doubles + 2 * M,), sentinel, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().pesr_ssim_y(ins[0].data_ptr() + 4 * M, ins[1].data_ptr() + 4 * M, out.data_ptr() + 8 * M, n, h, w, 0, 0, shave,
                                smap.data_ptr() + 8 * M, ws.data_ptr() + 8 * M, 8 * ws_doubles, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, used in ((out, n), (smap, n * ho * wo), (ws, ws_doubles)):
        assert bool((buf[:M] == sentinel).all()) and bool((buf[M + used:] == sentinel).all())
    got = smap[M:M + n * ho * wo].reshape(n, ho, wo).cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], SO.ssim_map(a[i], b[i], shave))
    assert torch.equal(out[M:M + n], ops.ssim_y(_to_dev(a, "c"), _to_dev(b, "c"), shave))
    # the C ABI's own refusals: nothing is launched, nothing is written
    lib = _lib.lib()
    args = (ins[0].data_ptr() + 4 * M, ins[1].data_ptr() + 4 * M, out.data_ptr() + 8 * M)
    assert lib.pesr_ssim_y(*args, n, h, w, 0, 0, 18, None, ws.data_ptr() + 8 * M, 8 * ws_doubles, stream) == -1    # 9 x 34 left
    assert lib.pesr_ssim_y(*args, n, h, w, 0, 0, -1, None, ws.data_ptr() + 8 * M, 8 * ws_doubles, stream) == -1
    assert lib.pesr_ssim_y(*args, 0, h, w, 0, 0, 0, None, ws.data_ptr() + 8 * M, 8 * ws_doubles, stream) == -1
    assert lib.pesr_ssim_y(*args, n, h, w, 0, 0, shave, None, ws.data_ptr() + 8 * M, 8, stream) == -2               # workspace too small
    assert lib.pesr_ssim_y(*args, n, h, w, 0, 0, shave, None, None, 0, stream) == -2
    torch.cuda.synchronize()
    assert bool((out[:M] == sentinel).all()) and bool((out[M + n:] == sentinel).all())


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (5 * x + 2 * y) // 2 % 256], axis=2).astype(np.uint8)


def _blocky(h, w, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 5) // 6, (w + 5) // 6, 3))
    return np.kron(base, np.ones((6, 6, 1), dtype=np.int64))[:h, :w].astype(np.uint8)


def _host_psnr_y(a, b):
    """utils.compute_PSNR's host formula on two uint8 HWC arrays."""
    coef = np.array([65.738, 129.057, 25.064]) / 256.0
    ya = np.clip(np.dot(a.astype(np.float64), coef) + 16, 0, 255).round()
    yb = np.clip(np.dot(b.astype(np.float64), coef) + 16, 0, 255).round()
    return 20 * np.log10(255 / np.sqrt(np.mean((ya - yb) ** 2)))


def _chw(img):
    return img.transpose(2, 0, 1).astype(np.float32)


@pytest.mark.parametrize("s", [4, 2])
def test_test_entrypoint_ssim_and_shave(tmp_path, monkeypatch, capsys, s):
    """test.py --from_hr true --ssim true --shave -1 on an HR-only folder of three PNGs (a 64-channel, 2-block seeded Generator)."""
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    spec = importlib.util.spec_from_file_location(f"entry_test_ssim{s}", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    hrs = {"a.png": _ramp(12 * s + 1, 10 * s + s - 1), "b.png": _rand(9 * s, 14 * s, 5), "c.png": _blocky(16 * s + 1, 11 * s, 6)}
    for name, im in hrs.items():
        Image.fromarray(im).save(base / "HR" / name)
    torch.save(gen_sd_scaled(64, 2, s, seed=3), tmp_path / "g.pt")
    common = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "64", "--num_blocks", "2", "--scale", str(s),
              "--from_hr", "true"]
    T.main(common + ["--ssim", "true", "--shave", "-1", "--save_path", str(tmp_path / "out")])
    text = capsys.readouterr().out
    num = r"([-\d.]+|inf)"
    seen = []
    for name, im in hrs.items():
        hr = RO.modcrop(im, s)
        sr = np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB"))
        bic = RO.imresize(RO.imresize(hr, s, False), s, True)
        m = re.search("^" + re.escape(name) + rf": PSNR-Y {num} dB, bicubic {num} dB, SSIM-Y {num}, bicubic {num}$", text, flags=re.M)
        assert m, text
        cut = lambda x: x[s:-s, s:-s]
        want = (_host_psnr_y(cut(sr), cut(hr)), _host_psnr_y(cut(bic), cut(hr)), SO.ssim(_chw(sr), _chw(hr), s), SO.ssim(_chw(bic), _chw(hr), s))
        print(f"x{s} {name}: printed {m.groups()}, restatement {want!r}")
        for k in range(4):
            assert abs(float(m.group(k + 1)) - want[k]) <= 1e-9          # (10 decimals are printed)
        assert re.fullmatch(r"0\.\d{10}|1\.0{10}|-0\.\d{10}", m.group(3)) and re.fullmatch(r"0\.\d{10}|1\.0{10}|-0\.\d{10}", m.group(4))
        seen.append(want)
    m = re.search(rf"^Mean PSNR-Y {num} dB, bicubic {num} dB, SSIM-Y {num}, bicubic {num}$", text, flags=re.M)
    assert m, text
    for k in range(4):
        assert abs(float(m.group(k + 1)) - np.mean([p[k] for p in seen])) <= 1e-9
    # without --ssim and --shave: exactly the lines of before, whole images
    capsys.readouterr()
    T.main(common + ["--save_path", str(tmp_path / "out2")])
    lines = [l for l in capsys.readouterr().out.splitlines() if not l.startswith("Number of parameters")]
    want_lines, means = [], []
    for i, (name, im) in enumerate(hrs.items()):
        hr = RO.modcrop(im, s)
        sr = np.asarray(Image.open(tmp_path / "out2" / "Toy" / name).convert("RGB"))
        assert np.array_equal(sr, np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB")))
        bic = RO.imresize(RO.imresize(hr, s, False), s, True)
        means.append((_host_psnr_y(sr, hr), _host_psnr_y(bic, hr)))
        want_lines += ["%s: PSNR-Y %.10f dB, bicubic %.10f dB" % ((name,) + means[-1]), "Tested %d img(s)" % (i + 1)]
    want_lines += ["Mean PSNR-Y %.10f dB, bicubic %.10f dB" % tuple(float(np.mean([p[k] for p in means])) for k in range(2)), "Finish"]
    assert len(lines) == len(want_lines)
    for got_line, want_line in zip(lines, want_lines):
        if got_line != want_line:                                         # the 10th decimal may round the other way: same form, same value
            form = re.sub(r"[-\d.]+ dB", "X dB", want_line)
            assert re.sub(r"[-\d.]+ dB", "X dB", got_line) == form and "SSIM" not in got_line
            for g, v in zip(re.findall(r"([-\d.]+) dB", got_line), re.findall(r"([-\d.]+) dB", want_line)):
                assert abs(float(g) - float(v)) <= 1e-9
    # the refusal
    with pytest.raises(SystemExit, match="--from_hr true"):
        T.main(["--dataset", "Toy", "--ssim", "true"])


def test_train_entrypoint_valid_ssim(tmp_path):
    """train.py --synthetic --valid_ssim true prints both validation lines; without the flag only the first (fresh interpreter)."""
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
common = ["--synthetic", "16", "--num_channels", "64", "--num_blocks", "2", "--patch_size", "8", "--batch_size", "4", "--num_epochs", "1",
          "--max_iters", "2", "--phase", "pretrain"]
Tm.main(common + ["--check_point", {ck!r} + "/a", "--valid_ssim", "true", "--valid_shave", "4"])
print("SECOND_RUN")
Tm.main(common + ["--check_point", {ck!r} + "/b"])
print("ENTRY_OK")
"""
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    first, second = r.stdout.split("SECOND_RUN")
    lines = first.splitlines()
    k = [i for i, l in enumerate(lines) if re.fullmatch(r"Finish valid \[1/1\]\. PSNR: [-\d.]+dB", l)]
    assert len(k) == 1, first[-2000:]
    m = re.fullmatch(r"Finish valid \[1/1\]\. SSIM: ([-\d.]+)", lines[k[0] + 1])
    assert m and -1.0 <= float(m.group(1)) <= 1.0, first[-2000:]
    assert re.search(r"^Finish valid \[1/1\]\. PSNR: [-\d.]+dB$", second, flags=re.M) and "SSIM" not in second
    assert (tmp_path / "ck" / "a" / "pretrain" / "best_model.pt").exists()
