"""GPU: LPIPS (docs/modes.md section 4n).

The head (pesr_amd/csrc/lpips.hip through ops.lpips_layer) against tests/lpips_oracle.py head_ordered BIT FOR BIT, map and score: the
kernel's order of operations is fixed and nothing is fused, so kernel and restatement perform the same IEEE operations.  How far
head_ordered is from the exactly summed definition is bounded on the CPU (tests/test_lpips_cpu.py), so the head needs no tolerance
here.

The whole metric (pesr_amd.lpips.lpips with LpipsModel.random) against lpips_f64.  Here the fp32 conv arithmetic of the trunk is the
limit, so the tolerance is measured and not chosen.  SCORE_RTOL (tests/lpips_cases.py): on the CPU the same cases with a float32 trunk
of direct convs differ from lpips_f64 by at most 1.218e-07 relative, at (1, 3, 16, 16) shave 0
(tests/test_lpips_cpu.py::test_float32_trunk_against_float64).  The tolerance is 16 times that, 1.949e-06: the device's Winograd F(4,3)
transforms add rounding that the direct convs do not have, and the cases sample it and do not bound it.  Every restated score is
above 1e-3 (asserted on the restatement alone), so a relative tolerance means something.  Then the users: utils.compute_LPIPS,
test.py --lpips and train.py --valid_lpips."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import lpips_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


# ---- the head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,h,w", C.HEAD_CASES)
def test_head_bit_for_bit(c, n, h, w):
    from pesr_amd import ops
    for kind in C.KINDS:
        fa, fb, wt = C.head_case(c, n, h, w, kind)
        want_score, want_map = C.head_answers(c, n, h, w, kind)["ordered"]
        feat, wd = _dev(np.concatenate([fa, fb])), _dev(wt)
        score, dmap = ops.lpips_layer(feat, wd, return_map=True)
        assert score.dtype == dmap.dtype == torch.float64 and score.shape == (n,) and dmap.shape == (n, h, w)
        plain = ops.lpips_layer(feat, wd)
        again = ops.lpips_layer(feat, wd, return_map=True)
        assert torch.equal(plain, score)                              # the score does not depend on whether the map is asked for
        assert torch.equal(again[0], score) and torch.equal(again[1], dmap)                   # the same bits on every call
        got_score, got_map = score.cpu().numpy(), dmap.cpu().numpy()
        assert not np.isnan(got_map).any() and not np.isnan(got_score).any()
        if not np.array_equal(got_map, want_map):
            bad = np.argwhere(got_map != want_map)
            pytest.fail(f"C {c} {n} x {h} x {w} {kind}: {len(bad)} of {want_map.size} elements of the map differ, first at {bad[0].tolist()}: "
                        f"{got_map[tuple(bad[0])]!r} != {want_map[tuple(bad[0])]!r}, max |diff| {np.max(np.abs(got_map - want_map)):.3e}")
        assert np.array_equal(got_score, want_score), f"C {c} {n} x {h} x {w} {kind}: score {got_score!r} != {want_score!r}"
        if kind == "same":
            assert bool((dmap == 0).all()) and bool((score == 0).all())


def test_head_margins_and_refusals():
    """Input surrounded by NaN (a read outside would poison the map), outputs and workspace surrounded by a sentinel; then the
    refusals: C = 96, a view (ops._chk takes contiguous tensors only, as for every NHWC op), a CPU tensor, an odd batch."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    M, sentinel = 4096, -12345.678
    for (c, n, h, w) in ((64,) + C.BIG_SHAPE, (512, 3, 9, 7)):
        fa, fb, wt = C.head_case(c, n, h, w, "relu")
        want_score, want_map = C.head_answers(c, n, h, w, "relu")["ordered"]
        f = np.concatenate([fa, fb])
        flat = torch.full((f.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
        flat[M:M + f.size] = _dev(f).reshape(-1)
        wflat = torch.full((c + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
        wflat[M:M + c] = _dev(wt)
        groups = (h * w + 63) // 64
        sizes = {"out": n, "map": n * h * w, "ws": n * groups}
        buf = {k: torch.full((v + 2 * M,), sentinel, dtype=torch.float64, device=DEV) for k, v in sizes.items()}
        ptr = {k: v.data_ptr() + 8 * M for k, v in buf.items()}
        rc = lib.pesr_lpips_layer(flat.data_ptr() + 4 * M, wflat.data_ptr() + 4 * M, ptr["out"], n, h, w, c, ptr["map"], ptr["ws"],
                                  8 * sizes["ws"], stream)
        assert rc == 0
        torch.cuda.synchronize()
        for k, v in buf.items():
            assert bool((v[:M] == sentinel).all()) and bool((v[M + sizes[k]:] == sentinel).all()), k
        assert np.array_equal(buf["out"][M:M + n].cpu().numpy(), want_score)
        assert np.array_equal(buf["map"][M:M + n * h * w].reshape(n, h, w).cpu().numpy(), want_map)
        keep = {k: v.clone() for k, v in buf.items()}
        for bad_c in (96, 32, 1024):
            assert lib.pesr_lpips_layer(flat.data_ptr() + 4 * M, wflat.data_ptr() + 4 * M, ptr["out"], n, h, w, bad_c, ptr["map"], ptr["ws"],
                                        8 * sizes["ws"], stream) == -1
        assert lib.pesr_lpips_layer(flat.data_ptr() + 4 * M, wflat.data_ptr() + 4 * M, ptr["out"], n, h, w, c, ptr["map"], ptr["ws"],
                                    8 * sizes["ws"] - 8, stream) == -2
        torch.cuda.synchronize()
        for k in buf:
            assert torch.equal(buf[k], keep[k]), k
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.lpips_layer(torch.zeros(2, 3, 5, 96, device=DEV), torch.ones(96, device=DEV))
    big = torch.zeros(4, 3, 5, 128, device=DEV)
    with pytest.raises(_lib.PesrHipError, match="contiguous"):
        ops.lpips_layer(big[:, :, :, :64], torch.ones(64, device=DEV))                          # a view in the channels
    with pytest.raises(_lib.PesrHipError, match="contiguous"):
        ops.lpips_layer(big[::2], torch.ones(128, device=DEV))                                  # a view in the batch
    with pytest.raises(_lib.PesrHipError):
        ops.lpips_layer(torch.zeros(3, 3, 5, 64, device=DEV), torch.ones(64, device=DEV))       # not [a; b]
    with pytest.raises(_lib.PesrHipError):
        ops.lpips_layer(torch.zeros(2, 3, 5, 64, device=DEV), torch.ones(128, device=DEV))
    with pytest.raises(_lib.PesrHipError):
        ops.lpips_layer(torch.zeros(2, 3, 5, 64), torch.ones(64))


def test_maxpool_forward_floors_odd_sides():
    """The trunk pools odd sides (37 -> 18, 9 -> 4): the forward drops the last row / column as nn.MaxPool2d(2) does; values are
    copied, so the comparison is exact.  The backward still takes even sides only."""
    import torch.nn.functional as F
    from pesr_amd import _lib, ops
    g = torch.Generator().manual_seed(4)
    for (n, h, w, c) in ((2, 37, 51, 64), (1, 9, 4, 128), (3, 3, 2, 512), (1, 2, 3, 4)):
        x = torch.randn(n, h, w, c, generator=g).to(DEV)
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        got = ops.maxpool2x2_fwd(x)
        assert got.shape == (n, h // 2, w // 2, c) and torch.equal(got, want)
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.maxpool2x2_fwd(torch.zeros(1, 1, 8, 64, device=DEV))
    # through autograd an odd side is refused at the forward when a gradient would be needed, and only then
    from pesr_amd import functional as PF
    odd = torch.rand(1, 5, 8, 64, device=DEV)
    assert PF.MaxPoolFn.apply(odd, True).shape == (1, 2, 4, 64)
    with pytest.raises(_lib.PesrHipError, match="even sides"):
        PF.MaxPoolFn.apply(odd.clone().requires_grad_(), True)
    even = torch.rand(1, 4, 8, 64, device=DEV).requires_grad_()
    PF.MaxPoolFn.apply(even, True).sum().backward()
    assert even.grad is not None and even.grad.shape == even.shape
    with pytest.raises(_lib.PesrHipError, match="PESR_EINVAL"):
        ops.maxpool2x2_bwd(torch.zeros(1, 5, 8, 64, device=DEV), torch.zeros(1, 2, 4, 64, device=DEV), False)


# ---- the whole metric --------------------------------------------------------------------------------------------------------------
def _layout(x, layout):
    t = _dev(x)
    if layout == "l":
        return t.contiguous(memory_format=torch.channels_last)
    if layout == "v":                                                # a view in neither layout
        big = torch.full((t.shape[0], 3, t.shape[2] + 5, t.shape[3] + 7), float("nan"), dtype=torch.float32, device=DEV)
        big[:, :, 2:2 + t.shape[2], 3:3 + t.shape[3]] = t
        return big[:, :, 2:2 + t.shape[2], 3:3 + t.shape[3]]
    return t.contiguous()


def _trunk_conv_shapes(h, w):
    """[(H, W, Cin, Cout)] of the 13 convs of the trunk for an h x w image."""
    from pesr_amd import lpips as LP
    out, c = [], 3
    for v in LP.CFG:
        if v == "M":
            h, w = h // 2, w // 2
        else:
            out.append((h, w, c, v))
            c = v
    return out


@pytest.mark.parametrize("shape,shave", C.METRIC_CASES)
def test_metric_against_the_float64_restatement(shape, shave):
    from pesr_amd import lpips as LP
    from pesr_amd import ops
    a, b = C.image_pair(shape)
    want = C.metric_f64(shape, shave)
    assert bool((want > C.MIN_SCORE).all())                           # on the restatement alone
    model = C.model()
    first = None
    for layout in ("c", "l", "v"):
        ta, tb = _layout(a, layout), _layout(b, layout)
        got = LP.lpips(ta, tb, model, shave)
        assert got.dtype == torch.float64 and got.shape == (shape[0],) and got.is_cuda
        rel = float(np.max(np.abs(got.cpu().numpy() - want) / want))
        print(f"{shape} shave {shave} layout {layout}: LPIPS {got.tolist()}, restatement {want.tolist()}, relative difference {rel:.3e}, "
              f"tolerance {C.SCORE_RTOL:.3e}")
        assert rel <= C.SCORE_RTOL
        if first is None:
            first = got
        assert torch.equal(first, got)                                # whatever the layout
        assert torch.equal(LP.lpips(ta, tb, model, shave), got)       # and on every call
        same = LP.lpips(ta, ta, model, shave)
        assert bool((same == 0.0).all()), same.tolist()
        back = LP.lpips(tb, ta, model, shave).cpu().numpy()
        assert float(np.max(np.abs(back - want) / want)) <= C.SCORE_RTOL
        assert float(np.max(np.abs(back - got.cpu().numpy()) / want)) <= C.SCORE_RTOL      # lpips(a, b) against lpips(b, a) directly
    score, maps = LP.lpips(_layout(a, "c"), _layout(b, "c"), model, shave, return_maps=True)
    assert torch.equal(score, first) and len(maps) == 5
    h, w = shape[2] - 2 * shave, shape[3] - 2 * shave
    total = torch.zeros_like(score)
    for m in maps:
        assert m.shape == (shape[0], h, w) and m.dtype == torch.float64
        total = total + m.mean(dim=(1, 2))
        h, w = h // 2, w // 2
    assert torch.allclose(total, score, rtol=1e-12, atol=0)
    # bf16 mode: the metric is measured with the fp32 kernels all the same, and the mode is restored.  The workgroup floor is lowered
    # as tests/test_bf16_gpu.py does, so that these small shapes WOULD take the bf16 kernels (asserted), and a trunk conv runs in
    # bf16 first, so that its weight cache holds a bf16 pack beside the fp32 one.
    n2, h, w = 2 * shape[0], shape[2] - 2 * shave, shape[3] - 2 * shave
    old = (ops.PRECISION, ops.BF16_MIN_WGS)
    ops.set_precision("bf16")
    ops.BF16_MIN_WGS = 1
    try:
        eligible = [i for i, (hh, ww, cin, cout) in enumerate(_trunk_conv_shapes(h, w)) if ops.bf16_eligible(n2, hh, ww, cin, cout)]
        print(f"{shape} shave {shave}: trunk convs that would run in bf16: {eligible}")
        assert eligible
        i = eligible[0]
        hh, ww, cin, cout = _trunk_conv_shapes(h, w)[i]
        x = torch.rand(n2, cin, hh, ww, generator=torch.Generator().manual_seed(3)).to(DEV).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            y16 = model.convs[i](x, act=ops.ACT_RELU).clone()
        got = LP.lpips(_layout(a, "c"), _layout(b, "c"), model, shave)
        assert ops.PRECISION == "bf16" and ops.BF16_MIN_WGS == 1
        ops.set_precision("fp32")
        with torch.no_grad():
            y32 = model.convs[i](x, act=ops.ACT_RELU)
        assert not torch.equal(y16, y32)                              # the bf16 kernel did run on that conv, and it is another kernel
    finally:
        ops.PRECISION, ops.BF16_MIN_WGS = old
    assert torch.equal(got, first)


def test_compute_lpips_and_refusals(tmp_path):
    import utils
    from pesr_amd import lpips as LP
    shape = (2, 3, 37, 51)
    a, b = C.image_pair(shape)
    ta, tb = _layout(a, "c"), _layout(b, "l")
    model = C.model()
    model.save(tmp_path / "w.pt")
    for shave in (0, 3):
        want = float(LP.lpips(ta, tb, model, shave).mean())
        assert utils.compute_LPIPS(ta, tb, model, shave) == want
        assert abs(want - float(C.metric_f64(shape, shave).mean())) <= C.SCORE_RTOL * want
    assert utils.compute_LPIPS(ta, tb, str(tmp_path / "w.pt"), 3) == want
    with pytest.raises(ValueError, match="differ in shape"):
        LP.lpips(ta, tb[:, :, :36], model)
    with pytest.raises(ValueError, match="16 x 16"):
        LP.lpips(ta[:, :, :15], tb[:, :, :15], model)
    with pytest.raises(ValueError, match="16 x 16"):
        LP.lpips(ta, tb, model, shave=11)                             # 37 - 22 = 15
    assert LP.lpips(ta, tb, model, shave=10).shape == (2,)            # 17 x 31
    with pytest.raises(ValueError, match="shave"):
        LP.lpips(ta, tb, model, shave=-1)
    small = _layout(C.image_pair((1, 3, 16, 16))[0], "c")            # 16 x 16 has no shave 3 case: 10 x 10 is below the four pools
    with pytest.raises(ValueError, match="16 x 16"):
        LP.lpips(small, small, model, shave=3)
    with pytest.raises(ValueError, match="no CPU path"):
        utils.compute_LPIPS(ta.cpu(), tb, model)
    with pytest.raises(ValueError, match="no CPU path"):
        LP.lpips(ta.double(), tb.double(), model)


def _chw(img):
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None].astype(np.float32)).to(DEV)


def test_test_entrypoint_lpips(tmp_path, monkeypatch, capsys):
    """test.py --from_hr true --lpips W on two 48 x 40 HR images (a 64-channel, 2-block seeded x4 Generator): per image and in the
    mean line the LPIPS of the saved result and of the bicubic baseline, equal to compute_LPIPS of the saved PNG (and of the restated
    bicubic image) against the HR image to the printed digits."""
    from PIL import Image
    import resize_oracle as RO
    from scale_oracle import gen_sd_scaled
    import utils
    spec = importlib.util.spec_from_file_location("entry_test_lpips", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    s = 4
    hr_dir = tmp_path / "data" / "origin" / "test" / "Toy" / "HR"
    hr_dir.mkdir(parents=True)
    rng = np.random.default_rng(21)
    hrs = {}
    for name in ("a.png", "b.png"):
        hr = np.clip(np.kron(rng.integers(30, 226, (6, 5, 3)), np.ones((8, 8, 1))) + rng.normal(0, 6, (48, 40, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(hr).save(hr_dir / name)
        hrs[name] = hr
    torch.save(gen_sd_scaled(64, 2, s, seed=3), tmp_path / "g.pt")
    model = C.model()
    model.save(tmp_path / "w.pt")
    common = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "64", "--num_blocks", "2", "--scale", str(s),
              "--from_hr", "true"]
    num = r"([-\d.]+|inf)"
    for shave in (0, 4):
        T.main(common + ["--lpips", str(tmp_path / "w.pt"), "--shave", str(shave), "--save_path", str(tmp_path / f"out{shave}")])
        text = capsys.readouterr().out
        means = []
        for name, hr in hrs.items():
            sr = np.asarray(Image.open(tmp_path / f"out{shave}" / "Toy" / name).convert("RGB"))
            assert sr.shape == hr.shape
            bic = RO.imresize(RO.imresize(hr, s, False), s, True)
            m = re.search(rf"^{re.escape(name)}: PSNR-Y {num} dB, bicubic {num} dB, LPIPS {num}, bicubic {num}$", text, flags=re.M)
            assert m, text
            want = (utils.compute_LPIPS(_chw(sr), _chw(hr), model, shave), utils.compute_LPIPS(_chw(bic), _chw(hr), model, shave))
            print(f"{name} shave {shave}: printed {m.group(3)}, {m.group(4)}; compute_LPIPS {want[0]!r}, {want[1]!r}")
            assert m.group(3) == "%.10f" % want[0] and m.group(4) == "%.10f" % want[1]
            assert want[0] > 0 and want[1] > 0
            means.append(want)
        m = re.search(rf"^Mean PSNR-Y {num} dB, bicubic {num} dB, LPIPS {num}, bicubic {num}$", text, flags=re.M)
        assert m, text
        assert m.group(3) == "%.10f" % float(np.mean([q[0] for q in means])) and m.group(4) == "%.10f" % float(np.mean([q[1] for q in means]))
    # after NIQE-less SSIM columns, and without the flag every line is what it was
    T.main(common + ["--ssim", "true", "--lpips", str(tmp_path / "w.pt"), "--save_path", str(tmp_path / "out_s")])
    assert re.search(rf"^a\.png: PSNR-Y {num} dB, bicubic {num} dB, SSIM-Y {num}, bicubic {num}, LPIPS {num}, bicubic {num}$",
                     capsys.readouterr().out, flags=re.M)
    T.main(common + ["--save_path", str(tmp_path / "out_n")])
    assert "LPIPS" not in capsys.readouterr().out


def test_train_entrypoint_valid_lpips(tmp_path):
    """train.py --synthetic --valid_lpips W prints the LPIPS line after the PSNR line; without the flag it does not (fresh interpreter)."""
    import subprocess
    import sys
    C.model().save(tmp_path / "w.pt")
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
common = ["--synthetic", "16", "--num_channels", "64", "--num_blocks", "2", "--patch_size", "8", "--batch_size", "4", "--num_epochs", "1",
          "--max_iters", "1", "--phase", "pretrain"]
Tm.main(common + ["--check_point", {ck!r} + "/a", "--valid_lpips", {str(tmp_path / "w.pt")!r}, "--valid_shave", "4"])
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
    m = re.fullmatch(r"Finish valid \[1/1\]\. LPIPS: ([-\d.]+)", lines[k[0] + 1])
    assert m and float(m.group(1)) > 0.0, first[-2000:]
    assert re.search(r"^Finish valid \[1/1\]\. PSNR: [-\d.]+dB$", second, flags=re.M) and "LPIPS" not in second
