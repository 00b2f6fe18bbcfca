"""GPU: NIQE block statistics (pesr_amd/csrc/niqe.hip through the C ABI, docs/modes.md section 4k) against the float64 restatement
of tests/niqe_oracle.py.  Both MSCN maps are compared BIT FOR BIT: the order of operations is fixed and nothing is fused, so kernel
and restatement perform the same IEEE operations.  Counts are equal.  Every sum is held to (n - 1) * 2^-53 relative to the exactly
summed (math.fsum) value, n the block's pixel count: all terms are non-negative, so that bound holds for any order of summation; it
is derived, not measured.  Then the host half (alpha grid indices, scores) fed the device's sums, and the users: utils.compute_NIQE
and test.py --niqe.

SCORE_RTOL: measured on the CPU (tests/niqe_cases.py perturbed_score_change): every sum of the restatement's stats moved by a random
sign times (n - 1) * 2^-53 relative, 20 draws per image of every case below; the largest relative change of the score was 3.831e-14
(96 x 192, B = 96, u8, gray).  The tolerance is 16 times that: the draws sample the worst case, they do not bound it."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import niqe_cases as C
import niqe_oracle as NO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
SCORE_RTOL = 16 * 3.831e-14
MIN_GAP = 1e-9
SUMS = [j for j in range(26) if j % 5 in (0, 2, 4)]          # (25, the sigma sum, is among them)
COUNTS = [j for j in range(25) if j % 5 in (1, 3)]


def _to_dev(x, layout):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if layout == "l":
        return t.contiguous(memory_format=torch.channels_last)
    if layout == "v":                                          # a view in neither layout: niqe_stats makes it contiguous
        big = torch.full((t.shape[0], 3, t.shape[2] + 5, t.shape[3] + 7), float("nan"), dtype=torch.float32, device=DEV)
        big[:, :, 2:2 + t.shape[2], 3:3 + t.shape[3]] = t
        return big[:, :, 2:2 + t.shape[2], 3:3 + t.shape[3]]
    return t.contiguous()


def _check_stats(got, want, B, what):
    """got, want: [2, nblk, 26]."""
    assert np.array_equal(got[:, :, COUNTS], want[:, :, COUNTS]), f"{what}: counts differ"
    for sc in range(2):
        n = (B >> sc) * (B >> sc)
        g, w = got[sc][:, SUMS], want[sc][:, SUMS]
        rel = np.abs(g - w) / np.where(w != 0, np.abs(w), 1.0)
        print(f"{what} scale {sc + 1}: largest relative error of a sum {rel.max():.3e}, bound {(n - 1) * 2.0 ** -53:.3e}")
        assert bool((rel <= (n - 1) * 2.0 ** -53).all()), f"{what} scale {sc + 1}: {rel.max():.3e}"
        assert bool((g[w == 0] == 0).all())


@pytest.mark.parametrize("luma", C.LUMAS)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("h,w,B,shave,n", C.SHAPES)
def test_maps_bit_for_bit_stats_indices_and_scores(h, w, B, shave, n, kind, luma):
    from pesr_amd import niqe as NQ
    a, res = C.case(h, w, B, shave, n, kind, luma)
    # the condition under which the alpha indices must agree, asserted on the restatement alone
    for i, r in enumerate(res):
        assert r["gap"] >= MIN_GAP, f"image {i}: the restatement's own smallest gap is {r['gap']:.3e}; choose another seed"
    model = NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, B, luma, 0)
    first = None
    for layout in (("c", "l", "v") if n > 1 else ("c", "l")):
        t = _to_dev(a, layout)
        stats, m1, m2 = NQ.niqe_stats(t, shave, B, luma, return_maps=True)
        nby, nbx = (h - 2 * shave) // B, (w - 2 * shave) // B
        assert stats.dtype == m1.dtype == m2.dtype == torch.float64 and stats.shape == (n, 2, nby * nbx, 26)
        assert m1.shape == (n, nby * B, nbx * B) and m2.shape == (n, nby * B // 2, nbx * B // 2)
        again = NQ.niqe_stats(t, shave, B, luma, return_maps=True)
        plain = NQ.niqe_stats(t, shave, B, luma)
        assert all(torch.equal(x, y) for x, y in zip(again, (stats, m1, m2)))          # deterministic: the same bits on every call
        assert torch.equal(plain, stats)                                                  # and with or without the map outputs
        if first is None:
            first = stats
        assert torch.equal(first, stats)                                                  # and whatever the layout
        stats, m1, m2 = stats.cpu().numpy(), m1.cpu().numpy(), m2.cpu().numpy()
        for i, r in enumerate(res):
            for name, got, want in (("scale-1", m1[i], r["m1"]), ("scale-2", m2[i], r["m2"])):
                if not np.array_equal(got, want):
                    bad = np.argwhere(got != want)
                    pytest.fail(f"image {i}, layout {layout}: {len(bad)} of {want.size} elements of the {name} MSCN map differ, first at "
                                f"{bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}, max |diff| "
                                f"{np.max(np.abs(got - want)):.3e}")
            _check_stats(stats[i], r["stats"], B, f"{h} x {w} B {B} {kind} {luma} image {i} layout {layout}")
        feat, index = NQ.features_from_stats(stats, B, return_index=True)
        for i, r in enumerate(res):
            assert np.array_equal(index[i], r["index"]), f"image {i}: alpha grid indices differ"
            if r["score"] is None:
                with pytest.raises(ValueError):
                    NQ.score(feat[i], model)
                continue
            got = NQ.score(feat[i], model)
            rel = abs(got - r["score"]) / r["score"]
            print(f"image {i} layout {layout}: NIQE {got!r}, restatement {r['score']!r}, relative difference {rel:.3e}, tolerance "
                  f"{SCORE_RTOL:.3e}")
            assert rel <= SCORE_RTOL
        scores = NQ.niqe(t, model, shave)
        assert len(scores) == n and all(isinstance(s, float) for s in scores)


def test_compute_niqe_device_path_margins_and_refusals(monkeypatch, tmp_path):
    import utils
    from pesr_amd import _lib
    from pesr_amd import niqe as NQ
    h, w, B, shave, n = 100, 131, 16, 4, 3
    a, res = C.case(h, w, B, shave, n, "float", "gray")
    model = NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, B, "gray", 0)
    model.save(tmp_path / "m.npz")
    # utils.compute_NIQE on a GPU tensor is the kernel (the mean over the images), on anything else the numpy route
    t = _to_dev(a, "l")
    calls = []
    real = NQ.niqe_stats
    monkeypatch.setattr(NQ, "niqe_stats", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    one = utils.compute_NIQE(t[:1], model, shave)
    every = utils.compute_NIQE(t, str(tmp_path / "m.npz"), shave)
    host = utils.compute_NIQE(t[:1].cpu(), model, shave)
    monkeypatch.undo()
    assert len(calls) == 2
    assert abs(one - res[0]["score"]) <= SCORE_RTOL * res[0]["score"]
    assert abs(every - np.mean([r["score"] for r in res])) <= SCORE_RTOL * every
    print(f"compute_NIQE: device {one!r}, numpy route {host!r}, relative difference {abs(host - one) / one:.3e}")
    assert abs(host - one) <= SCORE_RTOL * one
    # margins: the input surrounded by NaN (a read outside would poison a map), outputs and workspace surrounded by a sentinel
    M = 4096
    nby, nbx = (h - 2 * shave) // B, (w - 2 * shave) // B
    hc, wc = nby * B, nbx * B
    flat = torch.full((a.size + 2 * M,), float("nan"), dtype=torch.float32, device=DEV)
    flat[M:M + a.size] = torch.from_numpy(a).to(DEV).reshape(-1)
    sentinel = -12345.678
    sizes = {"stats": n * 2 * nby * nbx * 26, "m1": n * hc * wc, "m2": n * hc * wc // 4, "ws": 30 * n * hc * wc // 8}
    buf = {k: torch.full((v + 2 * M,), sentinel, dtype=torch.float64, device=DEV) for k, v in sizes.items()}
    ptr = {k: v.data_ptr() + 8 * M for k, v in buf.items()}
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    rc = lib.pesr_niqe_stats(flat.data_ptr() + 4 * M, n, h, w, 0, shave, B, 0, ptr["stats"], ptr["m1"], ptr["m2"], ptr["ws"], 8 * sizes["ws"],
                             stream)
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert bool((v[:M] == sentinel).all()) and bool((v[M + sizes[k]:] == sentinel).all()), k
    assert torch.equal(buf["stats"][M:M + sizes["stats"]].reshape(n, 2, nby * nbx, 26), NQ.niqe_stats(_to_dev(a, "c"), shave, B, "gray"))
    got1 = buf["m1"][M:M + sizes["m1"]].reshape(n, hc, wc).cpu().numpy()
    got2 = buf["m2"][M:M + sizes["m2"]].reshape(n, hc // 2, wc // 2).cpu().numpy()
    for i, r in enumerate(res):
        assert np.array_equal(got1[i], r["m1"]) and np.array_equal(got2[i], r["m2"])
    # the C ABI's own refusals: nothing is launched, nothing is written
    keep = {k: v.clone() for k, v in buf.items()}
    args = lambda **kw: [kw.get("img", flat.data_ptr() + 4 * M), kw.get("n", n), kw.get("h", h), kw.get("w", w), 0, kw.get("shave", shave),
                         kw.get("B", B), kw.get("luma", 0), ptr["stats"], ptr["m1"], ptr["m2"], kw.get("ws", ptr["ws"]),
                         kw.get("ws_bytes", 8 * sizes["ws"]), stream]
    for bad in ({"B": 15}, {"B": 6}, {"B": 98}, {"shave": -1}, {"n": 0}, {"n": 65536}, {"luma": 2}, {"luma": -1},
                {"h": 16 + 2 * shave, "w": 31 + 2 * shave},            # one block
                {"shave": 50}):                                        # nothing left
        assert lib.pesr_niqe_stats(*args(**bad)) == -1, bad
    assert lib.pesr_niqe_stats(*args(ws_bytes=8 * sizes["ws"] - 8)) == -2
    assert lib.pesr_niqe_stats(*args(ws=None, ws_bytes=0)) == -2
    torch.cuda.synchronize()
    for k in buf:
        assert torch.equal(buf[k], keep[k]), k
    # the Python layer's refusals
    big = _to_dev(a, "c")
    with pytest.raises(ValueError):
        NQ.niqe_stats(big, shave, 15)
    with pytest.raises(ValueError):
        NQ.niqe_stats(big, shave, 96)                                   # 92 x 123: one block of 96
    with pytest.raises(ValueError):
        NQ.niqe_stats(big, -1, B)
    with pytest.raises(ValueError):
        NQ.niqe_stats(big, shave, B, "luv")
    with pytest.raises(_lib.PesrHipError):
        NQ.niqe_stats(big.double(), shave, B)
    with pytest.raises(_lib.PesrHipError):
        NQ.niqe_stats(big.cpu(), shave, B)
    flat_img = torch.full((1, 3, 40, 40), 128.0, device=DEV)            # a constant image: every block is dropped
    with pytest.raises(ValueError, match="finite features"):
        NQ.niqe(flat_img, model)


def _chw(img):
    return img.transpose(2, 0, 1).astype(np.float32)


def test_test_entrypoint_niqe(tmp_path, monkeypatch, capsys):
    """test.py --niqe MODEL on one 32 x 48 LR image (a 64-channel, 2-block seeded x4 Generator, B = 16): with --from_hr true the NIQE
    columns are appended; without it, on an LR-only folder, a line per image carries NIQE alone."""
    from PIL import Image
    from scale_oracle import gen_sd_scaled
    from pesr_amd import niqe as NQ
    import utils
    spec = importlib.util.spec_from_file_location("entry_test_niqe", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    s = 4
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    (base / "LR").mkdir(parents=True)
    rng = np.random.default_rng(11)
    hr = np.clip(np.kron(rng.integers(30, 226, (16, 24, 3)), np.ones((8, 8, 1))) + rng.normal(0, 6, (128, 192, 3)), 0, 255).astype(np.uint8)
    lr = np.clip(np.kron(rng.integers(30, 226, (8, 12, 3)), np.ones((4, 4, 1))) + rng.normal(0, 6, (32, 48, 3)), 0, 255).astype(np.uint8)
    Image.fromarray(hr).save(base / "HR" / "a.png")
    Image.fromarray(lr).save(base / "LR" / "a.png")
    torch.save(gen_sd_scaled(64, 2, s, seed=3), tmp_path / "g.pt")
    model = NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, 16, "gray", 0)
    model.save(tmp_path / "m.npz")
    common = ["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "64", "--num_blocks", "2", "--scale", str(s)]
    num = r"([-\d.]+|inf)"

    def host(img, shave):
        return NO.niqe(_chw(img), C.MODEL_MU, C.MODEL_COV, shave, 16, "gray")

    # LR-only
    T.main(common + ["--niqe", str(tmp_path / "m.npz"), "--shave", "4", "--save_path", str(tmp_path / "out")])
    text = capsys.readouterr().out
    sr = np.asarray(Image.open(tmp_path / "out" / "Toy" / "a.png").convert("RGB"))
    assert sr.shape == (128, 192, 3)
    m = re.search(rf"^a\.png: NIQE {num}$", text, flags=re.M)
    assert m, text
    want = host(sr, 4)
    print(f"LR-only: printed {m.group(1)}, restatement {want!r}")
    assert abs(float(m.group(1)) - want) <= 1e-9 + SCORE_RTOL * want      # (10 decimals are printed)
    assert abs(float(m.group(1)) - utils.compute_NIQE(_chw(sr), model, 4)) <= 1e-9 + SCORE_RTOL * want
    m = re.search(rf"^Mean NIQE {num}$", text, flags=re.M)
    assert m and abs(float(m.group(1)) - want) <= 1e-9 + SCORE_RTOL * want, text
    # from HR
    T.main(common + ["--from_hr", "true", "--niqe", str(tmp_path / "m.npz"), "--save_path", str(tmp_path / "out2")])
    text = capsys.readouterr().out
    sr = np.asarray(Image.open(tmp_path / "out2" / "Toy" / "a.png").convert("RGB"))
    import resize_oracle as RO
    bic = RO.imresize(RO.imresize(hr, s, False), s, True)
    m = re.search(rf"^a\.png: PSNR-Y {num} dB, bicubic {num} dB, NIQE {num}, bicubic {num}$", text, flags=re.M)
    assert m, text
    for k, img in ((3, sr), (4, bic)):
        want = host(img, 0)
        assert abs(float(m.group(k)) - want) <= 1e-9 + SCORE_RTOL * want
        assert abs(float(m.group(k)) - utils.compute_NIQE(_chw(img), model, 0)) <= 1e-9 + SCORE_RTOL * want
    assert re.search(rf"^Mean PSNR-Y {num} dB, bicubic {num} dB, NIQE {num}, bicubic {num}$", text, flags=re.M), text
    # without the flag every line is what it was
    T.main(common + ["--save_path", str(tmp_path / "out3")])
    assert "NIQE" not in capsys.readouterr().out


def test_train_entrypoint_valid_niqe(tmp_path):
    """train.py --synthetic --valid_niqe MODEL prints the NIQE line after the PSNR line; without the flag it does not (fresh interpreter)."""
    import subprocess
    import sys
    from pesr_amd import niqe as NQ
    NQ.NiqeModel(C.MODEL_MU, C.MODEL_COV, 16, "gray", 0).save(tmp_path / "m.npz")
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
common = ["--synthetic", "16", "--num_channels", "64", "--num_blocks", "2", "--patch_size", "8", "--batch_size", "4", "--num_epochs", "1",
          "--max_iters", "2", "--phase", "pretrain"]
Tm.main(common + ["--check_point", {ck!r} + "/a", "--valid_niqe", {str(tmp_path / "m.npz")!r}])
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
    m = re.fullmatch(r"Finish valid \[1/1\]\. NIQE: ([-\d.]+)", lines[k[0] + 1])
    assert m and float(m.group(1)) > 0.0, first[-2000:]
    assert re.search(r"^Finish valid \[1/1\]\. PSNR: [-\d.]+dB$", second, flags=re.M) and "NIQE" not in second
    assert (tmp_path / "ck" / "a" / "pretrain" / "best_model.pt").exists()
