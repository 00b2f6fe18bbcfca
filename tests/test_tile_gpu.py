"""GPU: tiled inference (docs/modes.md section 4h).  The two kernels of csrc/tile.hip BIT FOR BIT against the restatement of
tests/tile_oracle.py (pure data movement and a handful of separately rounded fp32 operations: no excused element), the driver with
the exact toy model bit for bit against the whole-image result, the real Generator against the whole-image CPU oracle at the
tolerance test_generator_ragged_image_and_x8_ensemble uses for that comparison, the kernel family a tiled run dispatches to, and
the entry points."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tile_oracle as TO
from helpers import close, gen_sd, x8_toy_model
from oracle import detrand
from oracle import image as OI
from oracle import model as OM
from scale_oracle import gen_sd_scaled, generator_forward_scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
SENT = -12345.0


def _T():
    spec = importlib.util.spec_from_file_location("entry_test_tile", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    return T


def _G(C, depth, scale, sd):
    from model import Generator
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1, "scale": scale})
    G.load_state_dict(sd)
    return G.cuda()


def _img_u8(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- 6. gather ------------------------------------------------------------------------------------------------------------------------
def _gather_raw(src_t, u8, H, W, desc, oh, ow):
    """The C ABI with the source inside a NaN (0xFF for uint8) margin and the output inside a sentinel margin; -> the output."""
    from pesr_amd import _lib, ops
    pad = 4096
    n = len(desc)
    flat = src_t.contiguous().view(-1)
    if u8:
        big = torch.full((flat.numel() + 2 * pad,), 255, dtype=torch.uint8, device=DEV)
    else:
        big = torch.full((flat.numel() + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    big[pad:pad + flat.numel()] = flat
    out = torch.full((n * 3 * oh * ow + 2 * pad,), SENT, dtype=torch.float32, device=DEV)
    host = np.ascontiguousarray(np.array(desc, dtype=np.int32))
    dev = torch.from_numpy(host).to(DEV)
    rc = _lib.lib().pesr_tile_gather(big[pad:].data_ptr(), int(u8), H, W, out[pad:].data_ptr(), host.ctypes.data, dev.data_ptr(), n, oh, ow,
                                     ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out[:pad] == SENT).all()) and bool((out[pad + n * 3 * oh * ow:] == SENT).all())      # nothing outside the output
    return out[pad:pad + n * 3 * oh * ow].view(n, 3, oh, ow)


GATHER = [  # H, W, oh, ow: square and non-square tiles, odd image sizes, a tile that is the image, blocks above 32 in both directions
    (37, 53, 16, 16), (37, 53, 9, 20), (21, 70, 21, 32), (5, 7, 5, 7), (45, 70, 32, 32), (67, 131, 33, 65), (64, 64, 48, 48)]


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("H,W,oh,ow", GATHER)
def test_gather_bit_for_bit(H, W, oh, ow, u8):
    img = _img_u8(H, W, 100 + H + W)
    chw = torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32))
    desc = []
    for m in range(8):
        th, tw = (ow, oh) if m & 4 else (oh, ow)
        if th > H or tw > W:
            continue
        # every corner, an unaligned interior origin
        for y0, x0 in {(0, 0), (0, W - tw), (H - th, 0), (H - th, W - tw), ((H - th) // 2, min(max((W - tw) // 2 | 1, 0), W - tw))}:
            desc.append((y0, x0, m))
    src = torch.from_numpy(img).to(DEV) if u8 else chw.to(DEV)
    got = _gather_raw(src, u8, H, W, desc, oh, ow).cpu()
    want = TO.gather(chw, desc, oh, ow)
    assert not torch.isnan(got).any()
    assert torch.equal(got, want), [(i, desc[i]) for i in range(len(desc)) if not torch.equal(got[i], want[i])][:4]


def test_gather_large_source_and_ops_wrapper():
    from pesr_amd import _lib, ops
    H, W = 1356, 2040
    img = _img_u8(H, W, 9)
    chw = torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32))
    desc = [(0, 0, 0), (H - 96, W - 96, 3), (H - 96, 11, 5), (701, W - 96, 6), (1259, 1943, 7), (333, 777, 1), (3, 5, 2), (H - 96, W - 96, 4)]
    want = TO.gather(chw, desc, 96, 96)
    assert torch.equal(ops.tile_gather(torch.from_numpy(img).to(DEV), desc, 96, 96).cpu(), want)
    assert torch.equal(ops.tile_gather(chw.to(DEV), desc, 96, 96).cpu(), want)
    with pytest.raises(_lib.PesrHipError):
        ops.tile_gather(chw.to(DEV), [(H - 95, 0, 0)], 96, 96)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.tile_gather(chw, desc, 96, 96)


# ---- 7. scatter -----------------------------------------------------------------------------------------------------------------------
def _entries(n, h, w, seed, layout):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand((n, 3, h, w), generator=g) * 300.0 - 20.0).to(DEV)           # what a Generator puts out: -20 .. 280, non-integer
    return t.contiguous(memory_format=torch.channels_last) if layout == "l" else t


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("E,blend,layout", [(1, False, "c"), (1, True, "l"), (8, False, "l"), (8, True, "c")])
@pytest.mark.parametrize("H,W,core,halo", [(37, 53, 8, 3), (21, 40, 12, 5), (13, 9, 16, 2)])
def test_scatter_bit_for_bit(H, W, core, halo, E, blend, layout, s):
    from pesr_amd import ops, tile
    th, tw, desc = tile.plan(H, W, core, halo)
    k = len(desc)
    square = th == tw
    if E == 1:
        lo, hi = _entries(k, s * th, s * tw, 1, layout), None
        ent = [[lo[i]] for i in range(k)]
    elif square:
        lo, hi = _entries(8 * k, s * th, s * tw, 2, layout), None
        ent = [[lo[8 * i + m] for m in range(8)] for i in range(k)]
    else:
        lo, hi = _entries(4 * k, s * th, s * tw, 3, layout), _entries(4 * k, s * tw, s * th, 4, layout)
        ent = [[lo[4 * i + m] for m in range(4)] + [hi[4 * i + m] for m in range(4)] for i in range(k)]
    p = _entries(k, s * th, s * tw, 5, "l" if layout == "c" else "c") if blend else None
    wa, wb = tile.blend_weights(0.6) if blend else (1.0, 0.0)
    pad = 4096
    nf = 3 * s * H * s * W
    buf_f = torch.full((nf + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    buf_u = torch.full((nf + 2 * pad,), 77, dtype=torch.uint8, device=DEV)
    out_f, out_u = buf_f[pad:pad + nf].view(3, s * H, s * W), buf_u[pad:pad + nf].view(s * H, s * W, 3)
    ops.tile_scatter(lo, hi, desc, E, th, tw, s, H, W, out_f, out_u, p, wa, wb)
    torch.cuda.synchronize()
    assert not torch.isnan(out_f).any()                                           # every pixel written
    assert torch.isnan(buf_f[:pad]).all() and torch.isnan(buf_f[pad + nf:]).all()  # nothing outside the image
    assert bool((buf_u[:pad] == 77).all()) and bool((buf_u[pad + nf:] == 77).all())
    want = TO.scatter(ent, desc, E, th, tw, s, H, W, p, wa, wb)
    assert torch.equal(out_f, want), float((out_f - want).abs().max())
    assert torch.equal(out_u, TO.to_u8(want))
    again = torch.empty_like(want)
    ops.tile_scatter(lo, hi, desc, E, th, tw, s, H, W, again, None, p, wa, wb)
    assert torch.equal(again, out_f)                                              # the same bits on every run, with one output or both


def test_u8_rounds_half_to_even_and_clamps():
    from pesr_amd import ops
    vals = torch.tensor([-3.0, -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 127.49, 127.51, 0.0, 255.0], device=DEV)
    t = vals.repeat(3 * 4 * 4 * 4)[:3 * 16 * 16].view(1, 3, 16, 16).contiguous()
    out = torch.empty((16, 16, 3), dtype=torch.uint8, device=DEV)
    ops.tile_scatter(t, None, [(0, 0, 0, 0, 8, 8)], 1, 8, 8, 2, 8, 8, None, out)
    assert torch.equal(out, TO.to_u8(t[0]))
    assert set(out.unique().tolist()) == {0, 2, 127, 128, 254, 255}


# ---- 8. the driver with the exact toy model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,core,batch", [(37, 53, 8, 16), (9, 64, 16, 16), (13, 17, 32, 16), (40, 40, 8, 7)])
def test_driver_equals_whole_image_bit_for_bit(H, W, core, batch):
    """An image larger than the tile, one shorter than the tile on one axis (two shape groups in the ensemble) and one smaller than
    a tile; the padded last batch included - the model calls and their shapes are counted."""
    from pesr_amd import tile
    T = _T()
    inner = x8_toy_model(11, 12, "cuda")
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return inner(x)
    img = detrand.image_batch((1, 3, H, W), 400 + H).to(DEV)
    th, tw, tiles = tile.plan(H, W, core, 1)
    with torch.no_grad():
        whole, ens = inner(img), T.x8_forward(img, inner)
        got, got_u = tile.tiled_forward(model, img, 2, core, 1, batch, u8=True)
    assert torch.equal(got, whole) and torch.equal(got_u, TO.to_u8(whole[0]))
    n = len(tiles)
    if n > batch:
        assert calls == [(batch, 3, th, tw)] * (-(-n // batch))                    # one shape, the last batch padded
    else:
        assert calls == [(n, 3, th, tw)]
    del calls[:]
    u8_img = img[0].permute(1, 2, 0).contiguous().to(torch.uint8)                  # the uint8 HWC source form
    got, _ = tile.tiled_forward(model, u8_img, 2, core, 1, batch, ensemble=True)
    assert torch.equal(got, ens)
    per = max(batch // 8, 1)
    k = per if n > per else n
    rounds = -(-n // per)
    if th == tw:
        assert calls == [(8 * k, 3, th, tw)] * rounds
    else:
        assert calls == [(4 * k, 3, th, tw), (4 * k, 3, tw, th)] * rounds
    # the blend of test.py in one scatter
    other = x8_toy_model(21, 22, "cuda")
    with torch.no_grad():
        want = 0.6 * other(img) + (1 - 0.6) * ens
    got, _ = tile.tiled_forward(inner, img, 2, core, 1, batch, ensemble=True, blend_model=other, alpha=0.6)
    assert torch.equal(got, want)


# ---- 9. the real Generator against the whole-image CPU oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [4, 2, 3])
def test_generator_tiled_vs_whole_image_oracle(scale):
    from pesr_amd import tile
    sd = gen_sd_scaled(64, 2, scale, seed=5)
    G = _G(64, 2, scale, sd)
    img = detrand.image_batch((1, 3, 37, 53), 77)
    halo = tile.receptive_halo(2, scale)
    assert halo == 8
    fn = lambda t: generator_forward_scaled(sd, t, 2, 0.1, scale)
    with torch.no_grad():
        ref = fn(img)
        ens_ref = OI.x8_forward(img, fn)
    got, _ = tile.tiled_forward(G, img.to(DEV), scale, 8, halo, 16)
    close(got, ref, 1e-5, 2e-3, "tiled")
    ens, _ = tile.tiled_forward(G, img.to(DEV), scale, 8, halo, 16, ensemble=True)
    close(ens, ens_ref, 1e-5, 2e-3, "tiled x8")


# ---- 10. dispatch ---------------------------------------------------------------------------------------------------------------------
def test_tiled_run_stays_on_the_f43_kernels(monkeypatch):
    """C = 256, 1 block, LR 150 x 130, core 36, halo 6 (exact for 1 block), batch 16: 20 tiles of 48 x 48, two calls of
    [16, 3, 48, 48], the second padded; every 256 -> 256 and 256 -> 1024 conv of both calls runs with Wino4Packed weights."""
    from pesr_amd import ops, tile
    C = 256
    sd = gen_sd(C, 1, seed=9)
    G = _G(C, 1, 4, sd)
    assert tile.receptive_halo(1, 4) == 6
    th, tw, tiles = tile.plan(150, 130, 36, 6)
    assert (th, tw, len(tiles)) == (48, 48, 20)
    img = detrand.image_batch((1, 3, 150, 130), 4321).to(DEV)
    with torch.no_grad():
        whole = G(img)
    n = {"f43": 0, "other": 0}
    shapes = []
    inner, inner_fwd = ops._conv3x3_wino, ops.conv3x3_fwd

    def counted(x, wp, bias, skip, mask, y, N, H, W, cin, cout, *a, **k):
        if cin == C:
            n["f43" if isinstance(wp, ops.Wino4Packed) and (N, H, W) in ((16, 48, 48), (16, 96, 96)) else "other"] += 1
        return inner(x, wp, bias, skip, mask, y, N, H, W, cin, cout, *a, **k)

    def fwd(x, *a, **k):
        if x.shape[3] == C:
            shapes.append(tuple(x.shape))
        return inner_fwd(x, *a, **k)
    monkeypatch.setattr(ops, "_conv3x3_wino", counted)
    monkeypatch.setattr(ops, "conv3x3_fwd", fwd)
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        return G(x)
    got, _ = tile.tiled_forward(model, img, 4, 36, 6, 16)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls == [(16, 3, 48, 48)] * 2
    # per call: body.0's two convs, the trunk tail, upsample.0 and upsample.2 (the 256 -> 3 output conv has a kernel of its own)
    assert n == {"f43": 10, "other": 0}, (n, shapes)
    close(got, whole, 1e-5, 2e-3, "tiled vs whole image")


# ---- 11. the entry points -------------------------------------------------------------------------------------------------------------
def test_test_entrypoint_tiled_end_to_end(tmp_path, monkeypatch, capsys):
    from PIL import Image
    T = _T()
    monkeypatch.chdir(tmp_path)
    lr_dir = tmp_path / "data" / "origin" / "test" / "Toy" / "LR"
    lr_dir.mkdir(parents=True)
    imgs = {}
    for name, (h, w), seed in (("a.png", (45, 70), 1), ("b.png", (21, 70), 2)):
        arr = detrand.image_batch((h, w, 3), 900 + seed).numpy().astype(np.uint8)
        Image.fromarray(arr).save(lr_dir / name)
        imgs[name] = arr
    sd_perc, sd_psnr = gen_sd(64, 2, seed=3), gen_sd(64, 2, seed=4)
    torch.save(sd_perc, tmp_path / "perc.pt"); torch.save(sd_psnr, tmp_path / "psnr.pt")
    T.main(["--dataset", "Toy", "--perceptual_model", str(tmp_path / "perc.pt"), "--psnr_model", str(tmp_path / "psnr.pt"),
            "--num_channels", "64", "--num_blocks", "2", "--alpha", "0.6", "--save_path", str(tmp_path / "out"),
            "--tile", "16", "--tile_halo", "-1", "--tile_batch", "8"])
    text = capsys.readouterr().out
    assert "Tiled: tiles of 32 x 32" in text and "core 16, halo 8, exact halo 8" in text and "APPROXIMATION" not in text
    for name, arr in imgs.items():
        got = np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB")).astype(np.int32)
        x = torch.from_numpy(arr.transpose(2, 0, 1)[None].astype(np.float32))
        with torch.no_grad():
            ref = 0.6 * OM.generator_forward(sd_perc, x, 2, 0.1) + 0.4 * OI.x8_forward(x, lambda t: OM.generator_forward(sd_psnr, t, 2, 0.1))
        want = OI.tensor_to_img(ref).astype(np.int32)
        assert got.shape == want.shape == (4 * arr.shape[0], 4 * arr.shape[1], 3)
        print(name, np.abs(got - want).max(), (got != want).mean())
        assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.01, (np.abs(got - want).max(), (got != want).mean())


def test_test_entrypoint_tiled_from_hr_lines(tmp_path, monkeypatch, capsys):
    from PIL import Image
    T = _T()
    monkeypatch.chdir(tmp_path)
    base = tmp_path / "data" / "origin" / "test" / "Toy"
    (base / "HR").mkdir(parents=True)
    for name, im in {"a.png": _img_u8(4 * 40 + 1, 4 * 52, 5), "b.png": _img_u8(4 * 24, 4 * 33 + 2, 6)}.items():
        Image.fromarray(im).save(base / "HR" / name)
    torch.save(gen_sd(64, 2, seed=3), tmp_path / "g.pt")
    T.main(["--dataset", "Toy", "--perceptual_model", str(tmp_path / "g.pt"), "--num_channels", "64", "--num_blocks", "2", "--from_hr", "true",
            "--ssim", "true", "--shave", "-1", "--save_path", str(tmp_path / "out"), "--tile", "16", "--tile_halo", "4"])
    text = capsys.readouterr().out
    assert "APPROXIMATION" in text and "halo 4, exact halo 8" in text
    num = r"[-\d.]+"
    for name in ("a.png", "b.png"):
        assert re.search(rf"^{name}: PSNR-Y {num} dB, bicubic {num} dB, SSIM-Y {num}, bicubic {num}$", text, flags=re.M), text
    assert re.search(rf"^Mean PSNR-Y {num} dB, bicubic {num} dB, SSIM-Y {num}, bicubic {num}$", text, flags=re.M), text


def test_train_entrypoint_valid_tile(tmp_path):
    ck = str(tmp_path / "ck")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({ROOT!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
Tm.main(["--synthetic", "16", "--num_channels", "64", "--num_blocks", "2", "--patch_size", "24", "--batch_size", "4", "--num_epochs", "1",
         "--max_iters", "2", "--phase", "pretrain", "--check_point", {ck!r}, "--valid_tile", "16"])
print("ENTRY_OK")
"""
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Finish valid [1/1]. PSNR:" in r.stdout
