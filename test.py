#!/usr/bin/env python3
"""SR inference entry point (counterpart of reference test.py): perceptual model, optional PSNR model with x8
self-ensemble, image-space blend `alpha*out + (1-alpha)*out_psnr`, PNG output.  Same flags as the reference
(test.py:13-33) plus --precision, --scale and --from_hr (a test set that ships HR images only: LR made on the device, PSNR-Y of the
result and of the bicubic baseline printed; --ssim adds SSIM-Y, --shave drops a border before both), --niqe (the no-reference NIQE
of every saved image against a pristine model, with or without --from_hr; docs/modes.md section 4k), --lpips (with --from_hr true:
the full-reference LPIPS of every saved image and of the bicubic baseline against HR; section 4n), --dists (likewise, the
texture-tolerant DISTS; section 4t) and --tile (every image as
batches of fixed-size tiles, docs/modes.md section 4h); device-agnostic plumbing; the
Generator itself runs on the MI355X kernels.
"""
import argparse
import glob
import os

import numpy as np
import torch

from utils import default_device, imgs_to_tensors, tensors_to_imgs


# (flag, type, default, help) - the reference's flags and defaults (reference test.py:15-33)
_FLAGS = [
    ("dataset", str, "Set5", "folder under data/origin/test/ with an LR/ sub-folder of PNGs (HR/ with --from_hr true)"),
    ("perceptual_model", str, "check_point/PESR/train/PERC_model.pt", "GAN-phase generator checkpoint"),
    ("psnr_model", str, "check_point/PESR/pretrain/PSNR_model.pt", "L1-pretrained generator checkpoint (used when alpha != 1)"),
    ("num_channels", int, 256, "generator width"),
    ("num_blocks", int, 32, "generator depth (residual blocks)"),
    ("res_scale", float, 0.1, "residual scaling"),
    ("alpha", float, 1, "image-space blend: alpha * perceptual + (1 - alpha) * x8-ensembled PSNR output"),
    ("save_path", str, "results", "output folder"),
]


def build_parser():
    parser = argparse.ArgumentParser(description="x4 (or x2 / x3) super-resolution of a folder of LR images")
    for name, typ, default, text in _FLAGS:
        parser.add_argument("--" + name, type=typ, default=default, help=text)
    # an addition (not a reference flag): the optional bf16-operand mode of the build, DESIGN.md section 4c
    parser.add_argument("--precision", type=str, default="fp32", choices=["fp32", "bf16", "split-bf16"],
                        help="bf16: the generator's 3x3 convs round their operands to bf16 (fp32 accumulation and tensors): ~3x faster, "
                             "pixel values differ from the fp32 result by <= 1 grey level on a small fraction of pixels")
    # an addition (not a reference flag): the upscaling factor of the checkpoints, docs/modes.md section 4e
    parser.add_argument("--scale", type=int, default=4, choices=[2, 3, 4],
                        help="upscaling factor of the generator checkpoints (4: the reference's; 2 / 3: EDSR-style upsamplers)")
    # an addition (not a reference flag): a test set that ships HR images only, docs/modes.md section 4f
    parser.add_argument("--from_hr", type=lambda x: str(x).lower() == "true", default=False,
                        help="read data/origin/test/<dataset>/HR/*.png instead of LR/: crop each to multiples of --scale, make its LR image on "
                             "the GPU by MATLAB-style bicubic resize, and print PSNR-Y of the result and of the bicubic baseline against HR")
    # additions (not reference flags): the other half of a super-resolution table entry, docs/modes.md section 4g
    parser.add_argument("--ssim", type=lambda x: str(x).lower() == "true", default=False,
                        help="with --from_hr true: also print SSIM-Y (11 x 11 Gaussian window, measured on the GPU) of the result and of "
                             "the bicubic baseline")
    parser.add_argument("--shave", type=int, default=0,
                        help="with --from_hr true: drop a border of this many pixels before PSNR-Y and SSIM-Y are measured; -1 means "
                             "--scale, the convention of the published tables")
    # an addition (not a reference flag): the no-reference half of the Perceptual Index, docs/modes.md section 4k
    parser.add_argument("--niqe", type=str, default="",
                        help="a NIQE pristine model (.npz from `python -m pesr_amd.niqe fit`, or the standard .mat): also print the NIQE "
                             "of every saved image (measured on the GPU, --shave applied), and of the bicubic baseline with --from_hr "
                             "true; needs no HR images")
    # an addition (not a reference flag): the full-reference perceptual score, docs/modes.md section 4n
    parser.add_argument("--lpips", type=str, default="",
                        help="with --from_hr true: an LPIPS weight file (from `python -m pesr_amd.lpips pack`): also print the LPIPS (v0.1, "
                             "VGG variant, measured on the GPU, --shave applied) of every saved image and of the bicubic baseline "
                             "against the HR image")
    # an addition (not a reference flag): the texture-tolerant full-reference score, docs/modes.md section 4t
    parser.add_argument("--dists", type=str, default="",
                        help="with --from_hr true: a DISTS weight file (from `python -m pesr_amd.dists pack`): also print the DISTS "
                             "(measured on the GPU, --shave applied) of every saved image and of the bicubic baseline against the HR image")
    # additions (not reference flags): tiled inference, docs/modes.md section 4h
    parser.add_argument("--tile", type=int, default=0,
                        help="run every image as batches of overlapping tiles of one fixed shape on the GPU: the side of the square of "
                             "LR pixels a tile owns; 0 (default) = off, one Generator call on the whole image")
    parser.add_argument("--tile_halo", type=int, default=-1,
                        help="with --tile: LR pixels of context around a tile's owned square; -1 = 2 * num_blocks + 4, from which on the "
                             "result equals the whole-image forward up to fp32 summation order; a smaller halo is an approximation")
    parser.add_argument("--tile_batch", type=int, default=16,
                        help="with --tile: tiles per Generator call (entries per call for the x8 ensemble: rounded down to a multiple of 8)")
    # additions (not reference flags): a fixed non-bicubic test degradation, docs/modes.md section 4j
    parser.add_argument("--degradation", type=str, default="bicubic", choices=["bicubic", "classical"],
                        help="with --from_hr true: how the LR image is made.  classical: LR = (HR blurred by a Gaussian kernel) subsampled, "
                             "plus noise, the same kernel for every image (the BD / DN rows of the published tables, by this project's "
                             "own definition)")
    parser.add_argument("--blur_sigma", type=str, default="0",
                        help="with --degradation classical: S, the Gaussian's standard deviation in HR pixels, or S1,S2,THETA for an "
                             "anisotropic one; 0 (default) = no blur, the narrowest legal kernel with equal weights")
    parser.add_argument("--noise_sigma", type=float, default=0.0,
                        help="with --degradation classical: standard deviation of the added noise in grey levels; 0 (default) = none")
    parser.add_argument("--degrade_seed", type=int, default=0,
                        help="with --degradation classical: the noise stream number (image i of the sorted folder takes stream seed + i)")
    # additions (not reference flags): JPEG compression of the LR image, docs/modes.md section 4l
    parser.add_argument("--jpeg_quality", type=str, default="",
                        help="with --from_hr true: Q in 1 .. 100 - the LR image (bicubic or classical) goes through a JPEG round trip on the "
                             "GPU at this quality before the Generator sees it; default: no compression")
    parser.add_argument("--jpeg_chroma", type=str, default="420", choices=["420", "444"],
                        help="with --jpeg_quality: chroma at half resolution in both directions (420, default) or at full resolution (444)")
    # addition (not a reference flag): a fixed resize jitter of the LR image, docs/modes.md section 4m
    parser.add_argument("--resize_jitter", type=str, default="",
                        help="with --degradation classical: R[,M1[,M2]] - every LR image is resized to R times its sides (0.125 .. 8) with "
                             "filter M1 and back with filter M2 (bicubic, bilinear or box; default bicubic) on the GPU, the noise added "
                             "after the resize, before the JPEG round trip; default: none")
    return parser


def resize_jitter(args):
    """--resize_jitter -> (r, m1, m2) (None: no jitter); SystemExit naming the flags.  No GPU is touched."""
    if not args.resize_jitter:
        return None
    if args.degradation != "classical":
        raise SystemExit("test.py: --resize_jitter is a step of the classical degradation: it needs --from_hr true --degradation classical")
    from pesr_amd.degrade import parse_resize_jitter
    return parse_resize_jitter(args.resize_jitter, "test.py")


def jpeg_quality(args):
    """--jpeg_quality -> its integer (0: no compression); SystemExit naming the flags.  No GPU is touched."""
    if not args.jpeg_quality:
        return 0
    if not args.from_hr:
        raise SystemExit("test.py: --jpeg_quality compresses the LR image made from an HR image: it needs --from_hr true")
    from pesr_amd.jpeg import parse_quality
    return parse_quality(args.jpeg_quality, "test.py", "--jpeg_quality", 1)[0]


def classical_kernel(args):
    """--degradation classical -> its blur kernel (None for bicubic); SystemExit naming the flags.  No GPU is touched."""
    if args.degradation != "classical":
        return None
    if not args.from_hr:
        raise SystemExit("test.py: --degradation classical degrades HR images: it needs --from_hr true")
    from pesr_amd.degrade import delta_kernel, gaussian_kernel, kernel_size, parse_sigma_list
    vals = parse_sigma_list(args.blur_sigma, "test.py", "--blur_sigma", (1, 3))
    s1, s2, theta = vals if len(vals) == 3 else (vals[0], vals[0], 0.0)
    if not (args.noise_sigma >= 0 and np.isfinite(args.noise_sigma)):
        raise SystemExit(f"test.py: --noise_sigma {args.noise_sigma} must be >= 0")
    if s1 == 0 and s2 == 0:
        return delta_kernel(args.scale)
    if not (s1 > 0 and s2 > 0 and np.isfinite(s1) and np.isfinite(s2)):
        raise SystemExit(f"test.py: --blur_sigma {args.blur_sigma}: positive standard deviations (or a single 0) expected")
    return gaussian_kernel(kernel_size(args.scale, max(s1, s2)), s1, s2, theta)


def check_checkpoint_scale(sd, scale, path):
    """A checkpoint whose upsampler belongs to another scale than --scale: SystemExit naming both (instead of load_state_dict's
    size-mismatch dump)."""
    from pesr_amd.model import scale_of_state_dict
    try:
        found = scale_of_state_dict(sd)
    except ValueError as e:
        raise SystemExit(f"test.py: {path}: {e}")
    if found != scale:
        raise SystemExit(f"test.py: {path} is a x{found} generator, but --scale is {scale}; pass --scale {found}")
    return sd


def load_generator(opt, path, scale):
    """The Generator of a checkpoint: its width, depth and scale are the flags', its channel attention (docs/modes.md section 4u) and its
    window-attention blocks (section 4w) with or without their LayerNorm (section 4x) are read from the checkpoint itself."""
    from model import Generator
    from pesr_amd.model import attention_of_state_dict, wattn_norm_of_state_dict, wattn_of_state_dict
    sd = check_checkpoint_scale(torch.load(path, map_location="cpu"), scale, path)
    try:
        reduction = attention_of_state_dict(sd)
        positions, wattn_dim = wattn_of_state_dict(sd)
        wattn_norm = wattn_norm_of_state_dict(sd)
    except ValueError as e:
        raise SystemExit(f"test.py: {path}: {e}")
    if reduction:
        opt = dict(opt, attention="ca", ca_reduction=reduction)
    if positions:
        # (Generator puts a block after every E-th residual block: the first one's index says E, and the others have to follow from it)
        from pesr_amd.model.pesr import wattn_positions
        every = positions[0] + 1
        if wattn_positions(every, opt["depth"]) != positions:
            raise SystemExit(f"test.py: {path}: its window-attention blocks follow the residual blocks {list(positions)}; a Generator of "
                             f"--num_blocks {opt['depth']} has them after {list(wattn_positions(every, opt['depth']))} (every "
                             f"{every}-th block) or not at all")
        opt = dict(opt, wattn_every=every, wattn_dim=wattn_dim, wattn_norm=wattn_norm)
    if reduction or positions:
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}     # (saved from an nn.DataParallel)
    model = Generator(dict(opt, scale=scale))
    model.load_state_dict(sd)
    return model


def has_wattn(*models):
    return any(getattr(m, "wattn", None) is not None for m in models)


def has_attention(*models):
    from pesr_amd.model.basic import ChannelAttention
    return any(isinstance(mod, ChannelAttention) for m in models if m is not None for mod in m.modules())


# the three generators of the 8-element dihedral group, in the reference's order (test.py:58-60), as tensor ops
_TRANSFORMS = {
    "vflip": lambda t: t.flip(3),         # reference 'vflip' reverses the W axis
    "hflip": lambda t: t.flip(2),         # reference 'hflip' reverses the H axis
    "transpose": lambda t: t.transpose(2, 3),
}


def x8_forward(img, model):
    """Self-ensemble over the 8 flips/transposes (reference test.py:45-74), done on-device instead of through
    numpy round-trips.  Inputs are built by applying vflip, hflip, transpose cumulatively; output i is mapped back
    with transpose (i > 3), hflip (i % 4 > 1), vflip (i odd), then the 8 are averaged."""
    inputs = [img]
    for name in ("vflip", "hflip", "transpose"):
        inputs.extend([_TRANSFORMS[name](t).contiguous() for t in inputs])
    outputs = [model(t) for t in inputs]
    for i in range(len(outputs)):
        o = outputs[i]
        if i > 3:
            o = _TRANSFORMS["transpose"](o)
        if i % 4 > 1:
            o = _TRANSFORMS["hflip"](o)
        if (i % 4) % 2 == 1:
            o = _TRANSFORMS["vflip"](o)
        outputs[i] = o
    total = outputs[0]
    for o in outputs[1:]:
        total = total + o
    return total / len(outputs)


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _write_png(path, img):
    from PIL import Image
    Image.fromarray(img).save(path)


def lr_from_hr(hr_img, scale, device, kernel=None, noise_sigma=0.0, noise_stream=0, jpeg_q=0, jpeg_420=True, jitter=None):
    """--from_hr: uint8 HWC HR array -> (LR, mod-cropped HR, bicubic x`scale` of the LR) as [1,3,H,W] float tensors on the device;
    both resizes run there (pesr_amd.resize, docs/modes.md section 4f).  With a blur kernel the LR image is the classical
    degradation of section 4j instead of the bicubic one; with jpeg_q the LR image, however made, then goes through the JPEG round
    trip of section 4l, and the bicubic baseline is the upscale of the compressed image.  With jitter = (r, m1, m2) the classical
    LR image goes through the resize round trip of section 4m before that, its noise added in the second resize; the baseline is
    then the upscale of the jittered (or jittered and compressed) image."""
    from pesr_amd.degrade import lr_image_u8
    from pesr_amd.resize import imresize_u8, modcrop
    hr = torch.from_numpy(np.array(modcrop(hr_img, scale))).to(device)
    lr = lr_image_u8(hr, scale, kernel, noise_sigma, noise_stream, jitter, jpeg_q, jpeg_420)
    bic = imresize_u8(lr, scale, up=True)
    return tuple(t.permute(2, 0, 1)[None].float().contiguous() for t in (lr, hr, bic))


def _score(scorer, path, img, hr=None):
    from pesr_amd.quality import ScoreError
    try:
        return scorer.score(img, hr)
    except ScoreError as e:
        raise ValueError(f"{os.path.basename(path)}: {e}") from None


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.scale != 4 and args.precision != "fp32":
        raise SystemExit(f"test.py: --precision {args.precision} is checked for --scale 4 only; use --precision fp32 with --scale {args.scale}")
    if args.precision != "fp32":
        from pesr_amd import ops as _ops
        _ops.set_precision(args.precision)
    if args.ssim and not args.from_hr:
        raise SystemExit("test.py: --ssim true needs --from_hr true: without the HR images there is nothing to compare the result with")
    if args.shave < -1:
        raise SystemExit(f"test.py: --shave is a border width in pixels (or -1 for --scale), got {args.shave}")
    shave = args.scale if args.shave == -1 else args.shave
    kernel = classical_kernel(args)
    jpeg_q = jpeg_quality(args)
    jitter = resize_jitter(args)
    from pesr_amd.quality import Scorer
    scorer = Scorer("test.py", args.ssim, shave, args.niqe, args.lpips, have_hr=args.from_hr, dists=args.dists)
    scored = bool(scorer.columns(args.from_hr))     # (an LR-only set has a score only with --niqe)
    from pesr_amd import tile as _tile
    tile_halo = _tile.check_flags("test.py", ("--tile", "--tile_halo", "--tile_batch"), args.tile, args.tile_halo, args.tile_batch,
                                  args.num_blocks, args.scale)
    device = default_device()
    lr_paths = sorted(glob.glob(os.path.join("data/origin/test/", args.dataset, "HR" if args.from_hr else "LR", "*.png")))
    if scorer.niqe_model is not None or scorer.lpips_model is not None or scorer.dists_model is not None:       # (the size comes from the PNG header: still no GPU)
        from PIL import Image
        for path in lr_paths:
            with Image.open(path) as im:
                w, h = im.size
            h, w = (h - h % args.scale, w - w % args.scale) if args.from_hr else (h * args.scale, w * args.scale)
            scorer.check_size(h, w, os.path.basename(path))
    opt = {"num_channels": args.num_channels, "depth": args.num_blocks, "res_scale": args.res_scale}
    model = load_generator(opt, args.perceptual_model, args.scale).to(device)
    print("Number of parameters:", sum(p.nelement() for p in model.parameters()))
    model_psnr = None
    if args.alpha != 1:
        model_psnr = load_generator(opt, args.psnr_model, args.scale).to(device)
    save_path = os.path.join(args.save_path, args.dataset)
    os.makedirs(save_path, exist_ok=True)
    rows = []           # per image: the scores of what was saved and, with --from_hr, of the bicubic baseline
    if args.tile:
        print(_tile.describe(args.tile, tile_halo, _tile.receptive_halo(args.num_blocks, args.scale),
                             attention=has_attention(model, model_psnr), wattn=has_wattn(model, model_psnr)))
    with torch.no_grad():
        for i, lr_path in enumerate(lr_paths):
            if args.from_hr:
                inp, hr, bic = lr_from_hr(_read_png(lr_path), args.scale, device, kernel, args.noise_sigma, args.degrade_seed + i,
                                          jpeg_q, args.jpeg_chroma == "420", jitter)
            else:
                [inp] = imgs_to_tensors([_read_png(lr_path)], device)
            if args.tile:
                # [gather, G, scatter] per batch of tiles; the blend and the uint8 conversion happen in the scatter kernel
                if model_psnr is not None:
                    _, img = _tile.tiled_forward(model_psnr, inp, args.scale, args.tile, tile_halo, args.tile_batch, ensemble=True,
                                                 blend_model=model, alpha=args.alpha, f32=False, u8=True)
                else:
                    _, img = _tile.tiled_forward(model, inp, args.scale, args.tile, tile_halo, args.tile_batch, f32=False, u8=True)
                img = img.cpu().numpy()
            else:
                out = model(inp)
                if model_psnr is not None:
                    out = args.alpha * out + (1 - args.alpha) * x8_forward(inp, model_psnr)
                [img] = tensors_to_imgs([out])
            _write_png(os.path.join(save_path, os.path.basename(lr_path)), img)
            if scored:
                # the scores of what was SAVED: the uint8 image back on the device (compute_PSNR rounds the same way itself); an LR-only
                # set has no HR image and no baseline, and its NIQE needs neither
                [sr] = imgs_to_tensors([img], device)
                rows.append([_score(scorer, lr_path, t, hr) for t in (sr, bic)] if args.from_hr else [_score(scorer, lr_path, sr)])
                print("%s: %s" % (os.path.basename(lr_path), scorer.test_line(*rows[-1])))
            print("Tested %d img(s)" % (i + 1))
    if rows:
        print("Mean " + scorer.test_line(*(scorer.mean(r) for r in zip(*rows))))
    print("Finish")


if __name__ == "__main__":
    main()
