"""GPU: DISTS (docs/modes.md section 4t).

The L2 pooling (pesr_amd/csrc/dists.hip through ops.l2pool_fwd) against l2pool_f64 of the device's own input, within the derived
first-order bound L2POOL_RTOL of tests/dists_oracle.py (8 * 2^-24 relative; not measured).

The head (ops.dists_layer) against tests/dists_oracle.py layer_ordered BIT FOR BIT, the five statistics and the contribution: the
kernels' order of operations is fixed and nothing is fused, so kernel and restatement perform the same IEEE operations.  How far
layer_ordered is from exactly summed statistics is bounded on the CPU (tests/test_dists_cpu.py), so the head needs no tolerance here.

The whole metric (pesr_amd.dists.dists with DistsModel.random) against dists_f64.  Here the fp32 conv arithmetic of the trunk is the
limit, so the tolerance is measured and not chosen.  SCORE_ATOL (tests/dists_cases.py): on the CPU the same cases with a float32 trunk
of direct convs differ from dists_f64 by at most 5.859e-08 absolute (tests/test_dists_cpu.py::test_float32_trunk_against_float64).
The tolerance is 16 times that, 9.374e-07, and absolute because the score is one minus a sum near one: the device's Winograd F(4,3)
transforms add rounding that the direct convs do not have, and the cases sample it and do not bound it.  Then the users:
utils.compute_DISTS, test.py --dists and train.py --valid_dists."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import dists_cases as C
import dists_oracle as DO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


# ---- the L2 pooling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c", C.L2POOL_CASES)
def test_l2pool_against_float64(n, h, w, c):
    from pesr_amd import ops
    x, want = C.l2pool_case(n, h, w, c)
    got = ops.l2pool_fwd(_dev(x))
    assert got.dtype == torch.float32 and got.shape == (n, (h + 1) // 2, (w + 1) // 2, c) and got.is_contiguous()
    assert torch.equal(ops.l2pool_fwd(_dev(x)), got)
    g = got.cpu().numpy().astype(np.float64)
    rel = float(np.max(np.abs(g - want) / want))
    print(f"{n} x {h} x {w} x {c}: largest relative difference {rel:.3e} = {rel * 2 ** 24:.2f} * 2^-24, allowed {DO.L2POOL_RTOL:.3e}")
    assert bool((want >= 1e-6 * (1 - 1e-9)).all()) and rel <= DO.L2POOL_RTOL
    zero = ops.l2pool_fwd(torch.zeros(n, h, w, c, device=DEV))
    assert bool((zero == float(np.float32(np.sqrt(1e-12)))).all())   # sqrt(1e-12) rounded to fp32, on every element
    if (n, h, w, c) == C.L2POOL_BIG:                                  # more output than one workgroup writes
        plan = ops.l2pool_plan(n, h, w, c)
        assert plan["blocks"] >= 3 and got[0].numel() > plan["floats_per_block"] and got.numel() % plan["floats_per_block"]


def test_l2pool_margins_and_refusals():
    """Input surrounded by NaN (a read outside would poison the output), output surrounded by a sentinel; then the refusals."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    M, sentinel = 4096, -12345.678
    for (n, h, w, c) in ((2, 5, 7, 64), (2, 3, 2, 512), C.L2POOL_BIG):
        x, want = C.l2pool_case(n, h, w, c)
        flat = torch.full((x.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
        flat[M:M + x.size] = _dev(x).reshape(-1)
        size = n * ((h + 1) // 2) * ((w + 1) // 2) * c
        out = torch.full((size + 2 * M,), sentinel, dtype=torch.float32, device=DEV)
        assert lib.pesr_l2pool_fwd(flat.data_ptr() + 4 * M, out.data_ptr() + 4 * M, n, h, w, c, stream) == 0
        torch.cuda.synchronize()
        assert bool((out[:M] == sentinel).all()) and bool((out[M + size:] == sentinel).all())
        assert torch.equal(out[M:M + size].reshape(want.shape), ops.l2pool_fwd(_dev(x)))
        keep = out.clone()
        for bad_c in (96, 32, 3):
            assert lib.pesr_l2pool_fwd(flat.data_ptr() + 4 * M, out.data_ptr() + 4 * M, n, h, w, bad_c, stream) == -1
        assert lib.pesr_l2pool_fwd(flat.data_ptr() + 4 * M + 4, out.data_ptr() + 4 * M, n, h, w, c, stream) == -1
        torch.cuda.synchronize()
        assert torch.equal(out, keep)
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: C = 96"):
        ops.l2pool_fwd(torch.zeros(2, 3, 5, 96, device=DEV))
    big = torch.zeros(4, 3, 5, 128, device=DEV)
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: expected a contiguous"):
        ops.l2pool_fwd(big[:, :, :, :64])                                                       # a view in the channels
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: expected a contiguous"):
        ops.l2pool_fwd(big[::2])                                                                # a view in the batch
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: expected float32"):
        ops.l2pool_fwd(big.double())
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: .*GPU"):
        ops.l2pool_fwd(torch.zeros(2, 3, 5, 64))
    with pytest.raises(_lib.PesrHipError, match=r"l2pool_fwd\.x: expected a \[N, H, W, C\]"):
        ops.l2pool_fwd(torch.zeros(3, 5, 64, device=DEV))


# ---- the head ----------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_restatement_s():
    from pesr_amd import ops
    for c in C.LAYER_CHANNELS:
        assert [ops.dists_plan(C.LAYER_N, h * w, c)["pixel_blocks"] for h, w in C.LAYER_SIZES] == [1, 1, 2, 3]
        assert ops.dists_plan(C.LAYER_N, 256, c)["pixel_blocks"] == 1     # so 257 is the smallest P that takes two blocks
        assert ops.dists_plan(C.LAYER_N, 257, c)["pixels_per_block"] == DO.BLOCK_PIX


@pytest.mark.parametrize("c,hw", C.LAYER_CASES)
def test_layer_bit_for_bit(c, hw):
    from pesr_amd import ops
    for kind in C.KINDS:
        fa, fb, alpha, beta = C.layer_case(c, hw, kind)
        want, want_stats = C.layer_ordered(c, hw, kind)
        feat, ad, bd = _dev(np.concatenate([fa, fb])), _dev(alpha), _dev(beta)
        out, stats = ops.dists_layer(feat, ad, bd, return_stats=True)
        assert out.dtype == stats.dtype == torch.float64 and out.shape == (C.LAYER_N,) and stats.shape == (C.LAYER_N, c, 5)
        plain = ops.dists_layer(feat, ad, bd)
        again = ops.dists_layer(feat, ad, bd, return_stats=True)
        assert torch.equal(plain, out)                                # the sum does not depend on whether the statistics are asked for
        assert torch.equal(again[0], out) and torch.equal(again[1], stats)                    # the same bits on every call
        got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
        assert not np.isnan(got).any() and not np.isnan(got_stats).any()
        if not np.array_equal(got_stats, want_stats):
            bad = np.argwhere(got_stats != want_stats)
            pytest.fail(f"C {c} {hw} {kind}: {len(bad)} of {want_stats.size} statistics differ, first at {bad[0].tolist()}: "
                        f"{got_stats[tuple(bad[0])]!r} != {want_stats[tuple(bad[0])]!r}")
        assert np.array_equal(got, want), f"C {c} {hw} {kind}: contribution {got!r} != {want!r}"
        if kind == "zero":                                           # a channel of exact zeros in both maps: S1 = S2 = 1
            one = torch.zeros(c, dtype=torch.float64, device=DEV)
            one[c - 1] = 1.0
            assert bool((ops.dists_layer(feat, one, one) == 2.0).all())
        # changing image 0 leaves image 1's bits alone
        other = feat.clone()
        other[0] = other[0] * 0.5 + 0.25
        other[C.LAYER_N] = other[C.LAYER_N] + 1.0
        o2, s2 = ops.dists_layer(other, ad, bd, return_stats=True)
        assert torch.equal(o2[1:], out[1:]) and torch.equal(s2[1:], stats[1:]) and not torch.equal(s2[0], stats[0])


def test_layer_margins_and_refusals():
    """Inputs surrounded by NaN (a read outside would poison the result), the outputs and the workspace surrounded by a sentinel; then
    the refusals: a C it does not take, a view, a CPU tensor, a wrong dtype, shapes that differ, an odd batch."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    M, sentinel = 4096, -12345.678
    for c, hw in ((64, (3, 191)), (512, (5, 7)), (3, (1, 257))):
        fa, fb, alpha, beta = C.layer_case(c, hw, "relu")
        want, want_stats = C.layer_ordered(c, hw, "relu")
        n, (h, w) = C.LAYER_N, hw
        f = np.concatenate([fa, fb])
        flat = torch.full((f.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
        flat[M:M + f.size] = _dev(f).reshape(-1)
        wts = {}
        for k, v in (("alpha", alpha), ("beta", beta)):
            wts[k] = torch.full((c + 2 * M,), float("nan"), dtype=torch.float64, device=DEV)
            wts[k][M:M + c] = _dev(v)
        ws_bytes = ops.dists_plan(n, h * w, c)["workspace_bytes"]
        sizes = {"out": n, "stats": n * c * 5, "ws": ws_bytes // 8}
        buf = {k: torch.full((v + 2 * M,), sentinel, dtype=torch.float64, device=DEV) for k, v in sizes.items()}
        ptr = {k: v.data_ptr() + 8 * M for k, v in buf.items()}
        call = lambda cc=c, nb=ws_bytes, feat=flat.data_ptr() + 4 * M: lib.pesr_dists_layer(
            feat, wts["alpha"].data_ptr() + 8 * M, wts["beta"].data_ptr() + 8 * M, ptr["out"], n, h, w, cc, ptr["stats"], ptr["ws"], nb, stream)
        assert call() == 0
        torch.cuda.synchronize()
        for k, v in buf.items():
            assert bool((v[:M] == sentinel).all()) and bool((v[M + sizes[k]:] == sentinel).all()), k
        assert np.array_equal(buf["out"][M:M + n].cpu().numpy(), want)
        assert np.array_equal(buf["stats"][M:M + n * c * 5].reshape(n, c, 5).cpu().numpy(), want_stats)
        keep = {k: v.clone() for k, v in buf.items()}
        for bad_c in (96, 32, 1024, 4):
            assert call(cc=bad_c) == -1
        assert call(nb=ws_bytes - 8) == -2
        torch.cuda.synchronize()
        for k in buf:
            assert torch.equal(buf[k], keep[k]), k
    one64, one128 = torch.ones(64, dtype=torch.float64, device=DEV), torch.ones(128, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: C = 96"):
        ops.dists_layer(torch.zeros(2, 3, 5, 96, device=DEV), torch.ones(96, dtype=torch.float64, device=DEV), torch.ones(96, dtype=torch.float64, device=DEV))
    big = torch.zeros(4, 3, 5, 128, device=DEV)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: expected a contiguous"):
        ops.dists_layer(big[:, :, :, :64], one64, one64)                                        # a view in the channels
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: expected a contiguous"):
        ops.dists_layer(big[::2], one128, one128)                                               # a view in the batch
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: expected a \[2N, H, W, C\]"):
        ops.dists_layer(torch.zeros(3, 3, 5, 64, device=DEV), one64, one64)                     # not [a; b]
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: expected float32"):
        ops.dists_layer(big.double(), one128, one128)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.beta: expected 64 weights"):
        ops.dists_layer(torch.zeros(2, 3, 5, 64, device=DEV), one64, one128)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.alpha: expected float64"):
        ops.dists_layer(torch.zeros(2, 3, 5, 64, device=DEV), one64.float(), one64)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.alpha: expected a contiguous"):
        ops.dists_layer(torch.zeros(2, 3, 5, 64, device=DEV), one128[::2], one64)
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.beta: .*GPU"):
        ops.dists_layer(torch.zeros(2, 3, 5, 64, device=DEV), one64, one64.cpu())
    with pytest.raises(_lib.PesrHipError, match=r"dists_layer\.feat: .*GPU"):
        ops.dists_layer(torch.zeros(2, 3, 5, 64), one64, one64)


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
    """[(H, W, Cin, Cout)] of the 13 convs of the trunk for an h x w image: the L2 pooling leaves ceil(side / 2)."""
    from pesr_amd import lpips as LP
    out, c = [], 3
    for v in LP.CFG:
        if v == "M":
            h, w = (h + 1) // 2, (w + 1) // 2
        else:
            out.append((h, w, c, v))
            c = v
    return out


@pytest.mark.parametrize("shape,shave", C.METRIC_CASES)
def test_metric_against_the_float64_definition(shape, shave):
    from pesr_amd import dists as DS
    from pesr_amd import ops
    a, b = C.image_pair(shape, shave)
    want, want_parts = C.metric_f64(shape, shave)
    model = C.model()
    first = None
    for layout in ("c", "l", "v"):
        ta, tb = _layout(a, layout), _layout(b, layout)
        got = DS.dists(ta, tb, model, shave)
        assert got.dtype == torch.float64 and got.shape == (shape[0],) and got.is_cuda
        diff = float(np.max(np.abs(got.cpu().numpy() - want)))
        print(f"{shape} shave {shave} layout {layout}: DISTS {got.tolist()}, definition {want.tolist()}, absolute difference {diff:.3e}, "
              f"tolerance {C.SCORE_ATOL:.3e}")
        assert diff <= C.SCORE_ATOL
        if first is None:
            first = got
        assert torch.equal(first, got)                                # whatever the layout
        assert torch.equal(DS.dists(ta, tb, model, shave), got)       # and on every call
        same = DS.dists(ta, ta, model, shave)
        assert float(same.abs().max()) <= 1475 * 2.0 ** -53, same.tolist()
        back = DS.dists(tb, ta, model, shave).cpu().numpy()
        assert float(np.max(np.abs(back - want))) <= C.SCORE_ATOL
    score, parts = DS.dists(_layout(a, "c"), _layout(b, "c"), model, shave, return_parts=True)
    assert torch.equal(score, first) and len(parts) == 6
    total = torch.zeros_like(score)
    for p, wp in zip(parts, want_parts):
        assert p.shape == (shape[0],) and p.dtype == torch.float64
        assert float(np.max(np.abs(p.cpu().numpy() - wp))) <= C.SCORE_ATOL
        total = total + p
    assert torch.equal(1.0 - total, score)                           # the parts sum, in stage order, to one minus the score
    # bf16 mode: the metric is measured with the fp32 kernels all the same, and the mode is restored.  The workgroup floor is lowered
    # as tests/test_bf16_gpu.py does, so that these small shapes WOULD take the bf16 kernels (asserted), and a trunk conv runs in
    # bf16 first, so that its weight cache holds a bf16 pack beside the fp32 one.
    n2, h, w = 2 * shape[0], shape[2], shape[3]
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
        got = DS.dists(_layout(a, "c"), _layout(b, "c"), model, shave)
        assert ops.PRECISION == "bf16" and ops.BF16_MIN_WGS == 1
        ops.set_precision("fp32")
        with torch.no_grad():
            y32 = model.convs[i](x, act=ops.ACT_RELU)
        assert not torch.equal(y16, y32)                              # the bf16 kernel did run on that conv, and it is another kernel
    finally:
        ops.PRECISION, ops.BF16_MIN_WGS = old
    assert torch.equal(got, first)


def test_compute_dists_and_refusals(tmp_path):
    import utils
    from pesr_amd import dists as DS
    shape = (2, 3, 17, 23)
    a, b = C.image_pair(shape, 2)                                    # 21 x 27
    ta, tb = _layout(a, "c"), _layout(b, "l")
    model = C.model()
    model.save(tmp_path / "w.pt")
    for shave in (0, 2):
        want = float(DS.dists(ta, tb, model, shave).mean())
        assert utils.compute_DISTS(ta, tb, model, shave) == want
    assert abs(want - float(C.metric_f64(shape, 2)[0].mean())) <= C.SCORE_ATOL
    assert utils.compute_DISTS(ta, tb, str(tmp_path / "w.pt"), 2) == want
    with pytest.raises(ValueError, match="differ in shape"):
        DS.dists(ta, tb[:, :, :20], model)
    with pytest.raises(ValueError, match="16 x 16"):
        DS.dists(ta[:, :, :15], tb[:, :, :15], model)
    with pytest.raises(ValueError, match="16 x 16"):
        DS.dists(ta, tb, model, shave=3)                              # 21 - 6 = 15
    with pytest.raises(ValueError, match="shave"):
        DS.dists(ta, tb, model, shave=-1)
    with pytest.raises(ValueError, match="no CPU path"):
        utils.compute_DISTS(ta.cpu(), tb, model)
    with pytest.raises(ValueError, match="no CPU path"):
        DS.dists(ta.double(), tb.double(), model)
    with pytest.raises(ValueError, match="an LPIPS weight file"):
        import lpips_cases as LC
        LC.model().save(tmp_path / "l.pt")
        utils.compute_DISTS(ta, tb, str(tmp_path / "l.pt"))


def _chw(img):
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None].astype(np.float32)).to(DEV)


def test_test_entrypoint_dists(tmp_path, monkeypatch, capsys):
    """test.py --from_hr true --dists W on two 48 x 40 HR images (a 64-channel, 2-block seeded x4 Generator): per image and in the mean
    line the DISTS of the saved result and of the bicubic baseline, equal to compute_DISTS of the saved PNG (and of the restated bicubic
    image) against the HR image to the printed digits; absent without the flag."""
    from PIL import Image
    import resize_oracle as RO
    from scale_oracle import gen_sd_scaled
    import utils
    spec = importlib.util.spec_from_file_location("entry_test_dists", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    s = 4
    hr_dir = tmp_path / "data" / "origin" / "test" / "Toy" / "HR"
    hr_dir.mkdir(parents=True)
    rng = np.random.default_rng(23)
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
    shave = 4
    T.main(common + ["--dists", str(tmp_path / "w.pt"), "--shave", str(shave), "--save_path", str(tmp_path / "out")])
    text = capsys.readouterr().out
    means = []
    for name, hr in hrs.items():
        sr = np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB"))
        assert sr.shape == hr.shape
        bic = RO.imresize(RO.imresize(hr, s, False), s, True)
        m = re.search(rf"^{re.escape(name)}: PSNR-Y {num} dB, bicubic {num} dB, DISTS {num}, bicubic {num}$", text, flags=re.M)
        assert m, text
        want = (utils.compute_DISTS(_chw(sr), _chw(hr), model, shave), utils.compute_DISTS(_chw(bic), _chw(hr), model, shave))
        print(f"{name} shave {shave}: printed {m.group(3)}, {m.group(4)}; compute_DISTS {want[0]!r}, {want[1]!r}")
        assert m.group(3) == "%.10f" % want[0] and m.group(4) == "%.10f" % want[1]
        assert want[0] > 0 and want[1] > 0
        means.append(want)
    m = re.search(rf"^Mean PSNR-Y {num} dB, bicubic {num} dB, DISTS {num}, bicubic {num}$", text, flags=re.M)
    assert m, text
    assert m.group(3) == "%.10f" % float(np.mean([q[0] for q in means])) and m.group(4) == "%.10f" % float(np.mean([q[1] for q in means]))
    # behind LPIPS when both are asked for, and without the flag every line is what it was
    import lpips_cases as LC
    LC.model().save(tmp_path / "l.pt")
    T.main(common + ["--lpips", str(tmp_path / "l.pt"), "--dists", str(tmp_path / "w.pt"), "--save_path", str(tmp_path / "out_b")])
    assert re.search(rf"^a\.png: PSNR-Y {num} dB, bicubic {num} dB, LPIPS {num}, bicubic {num}, DISTS {num}, bicubic {num}$",
                     capsys.readouterr().out, flags=re.M)
    T.main(common + ["--save_path", str(tmp_path / "out_n")])
    assert "DISTS" not in capsys.readouterr().out


def test_train_entrypoint_valid_dists(tmp_path):
    """train.py --synthetic --valid_dists W prints the DISTS line after the PSNR line; without the flag it does not (fresh interpreter)."""
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
Tm.main(common + ["--check_point", {ck!r} + "/a", "--valid_dists", {str(tmp_path / "w.pt")!r}, "--valid_shave", "4"])
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
    m = re.fullmatch(r"Finish valid \[1/1\]\. DISTS: ([-\d.]+)", lines[k[0] + 1])
    assert m and float(m.group(1)) > 0.0, first[-2000:]
    assert re.search(r"^Finish valid \[1/1\]\. PSNR: [-\d.]+dB$", second, flags=re.M) and "DISTS" not in second
