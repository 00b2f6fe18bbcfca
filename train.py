#!/usr/bin/env python3
"""Training entry point (counterpart of reference train.py) on the MI355X-native model package.

Same flags and defaults as the reference (train.py:21-77) plus `--synthetic N` (random DIV2K-shaped crops instead of
the DIV2K cache, which is out of scope here).  One process per GPU: run plainly for one GPU, or under
`python -m torch.distributed.run --nproc-per-node N train.py ...` for N (RCCL gradient all-reduce inside the
optimizers replaces nn.DataParallel; --batch_size stays the GLOBAL batch as in the reference, each rank takes 1/N).
tensorboardX is optional.  Checkpoints keep the reference's format: torch.save(G.state_dict()).  --save_state_every / --resume
add a full training state file next to them (pesr_amd/checkpoint.py), --ema_decay a moving average of G's weights.
"""
import argparse
import json
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.optim.lr_scheduler as lr_scheduler
from torch.utils.data import DataLoader, RandomSampler
from torch.utils.data.distributed import DistributedSampler


def str2bool(x):
    return str(x).lower() == "true"


def build_parser():
    p = argparse.ArgumentParser(description="PIRM 2018")
    p.add_argument("--scale", type=int, default=4,
                   help="interpolation scale: 4 (the reference's), or 2 / 3 (an extension: EDSR-style upsamplers, docs/modes.md section 4e)")
    p.add_argument("--train_dataset", type=str, default="DIV2K")
    p.add_argument("--valid_dataset", type=str, default="PIRM")
    p.add_argument("--num_valids", type=int, default=10)
    p.add_argument("--num_channels", type=int, default=256)
    p.add_argument("--num_blocks", type=int, default=32)
    p.add_argument("--res_scale", type=float, default=0.1)
    p.add_argument("--phase", type=str, default="train", help="pretrain or train")
    p.add_argument("--pretrained_model", type=str, default="")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--learning_rate", type=float, default=5e-5)
    p.add_argument("--lr_step", type=int, default=120)
    p.add_argument("--num_epochs", type=int, default=200)
    p.add_argument("--num_repeats", type=int, default=20)
    p.add_argument("--patch_size", type=int, default=24)
    p.add_argument("--check_point", type=str, default="check_point/my_model")
    p.add_argument("--snapshot_every", type=int, default=10)
    p.add_argument("--gan_type", type=str, default="RSGAN")
    p.add_argument("--GP", type=str2bool, default=False)
    p.add_argument("--spectral_norm", type=str2bool, default=False)
    p.add_argument("--focal_loss", type=str2bool, default=True)
    p.add_argument("--fl_gamma", type=float, default=1)
    p.add_argument("--alpha_vgg", type=float, default=50)
    p.add_argument("--alpha_gan", type=float, default=1)
    p.add_argument("--alpha_tv", type=float, default=1e-6)
    p.add_argument("--alpha_l1", type=float, default=0)
    # additions
    p.add_argument("--attention", type=str, default="none", choices=["none", "ca"],
                   help="ca: RCAN-style channel attention (a squeeze-and-excite gate on the second conv's output) in every residual "
                        "block of the Generator (docs/modes.md section 4u); none (default): the reference's blocks")
    p.add_argument("--ca_reduction", type=int, default=16,
                   help="with --attention ca: the gate's hidden width is --num_channels / this; it has to divide --num_channels")
    p.add_argument("--wattn_every", type=int, default=0,
                   help="E > 0: a window self-attention block (8 x 8 windows, heads of 32 channels, shifted by half a window at every "
                        "second block; docs/modes.md section 4w) after every E-th residual block of the Generator; 0 (default): none")
    p.add_argument("--wattn_dim", type=int, default=0,
                   help="with --wattn_every: the attention width, a multiple of 32 (the head width) up to 1024; 0 (default): "
                        "--num_channels / 2")
    p.add_argument("--wattn_norm", type=str, default="none", choices=["none", "ln"],
                   help="with --wattn_every: ln puts a LayerNorm over each pixel's channels in front of every block's qkv (the pre-norm of a "
                        "Swin layer; docs/modes.md section 4x), so that the attention does not start saturated; none (default): the "
                        "blocks without it")
    p.add_argument("--d_arch", type=str, default="vgg", choices=["vgg", "unet"],
                   help="unet: a U-Net discriminator with one logit per pixel (Real-ESRGAN's, with 3 x 3 stride-2 convs; docs/modes.md "
                        "section 4v), independent of --patch_size; vgg (default): the reference's Discriminator.  Unused in --phase pretrain")
    p.add_argument("--d_width", type=int, default=64,
                   help="with --d_arch unet: the channels of its first conv (a positive multiple of 16)")
    p.add_argument("--synthetic", type=int, default=0, help="train on N synthetic samples per epoch instead of a dataset folder")
    p.add_argument("--vgg_weights", type=str, default="",
                   help="state_dict file of torchvision's pretrained vgg19 (torch.save(torchvision.models.vgg19(pretrained=True)"
                        ".state_dict(), path)); REQUIRED for the GAN phase unless torchvision itself is importable")
    p.add_argument("--allow_random_vgg", type=str2bool, default=False,
                   help="GAN phase without pretrained VGG19 weights: seeded random features (benchmarks / smoke runs only - the "
                        "perceptual loss is then NOT the reference's)")
    p.add_argument("--max_iters", type=int, default=0, help="stop each epoch after this many iterations (smoke runs)")
    p.add_argument("--hip_graph", type=str, default="auto", choices=["auto", "true", "false", "True", "False"],
                   help="capture the train step into a hipGraph after two eager iterations and replay it (same results bit for "
                        "bit; the host no longer issues ~1000 launches per step).  auto = on for a single-GPU run; under "
                        "torch.distributed the captured step (RCCL all-reduces included) is one candidate of --dp_policy auto")
    p.add_argument("--dp_peer_candidate", type=str, default="true",
                   help="--dp_policy auto also times the CU-free gradient exchange over peer memory (pesr_amd/comm.py PeerCopy), after a "
                        "rehearsal in child processes; it replaces RCCL only if it is faster")
    p.add_argument("--dp_policy", type=str, default="auto", choices=["auto", "overlap", "defer_g", "defer_all"],
                   help="under torch.distributed: how the gradient all-reduces are scheduled against the backward kernels.  auto = "
                        "measured during the first iterations (Trainer.calibrate_dp_policy: eager overlap, G's exchange deferred behind "
                        "its backward pass, both deferred, and - unless --hip_graph false - the captured step) and the fastest kept")
    p.add_argument("--precision", type=str, default="fp32", choices=["fp32", "bf16", "split-bf16"],
                   help="fp32 (default): the reference's arithmetic.  bf16: OPTIONAL mixed-precision mode - the stride-1 3x3 convs with "
                        "32-multiple input / 64-multiple output channels run on the bf16 MFMA (both operands rounded to bf16, fp32 "
                        "accumulation, fp32 tensors and optimizer): ~2.4x the step rate, NOT the reference's numerics.  split-bf16: "
                        "OPTIONAL - forward and input gradient of the stride-1 convs with Cout % 128 == 0 as THREE bf16 products per "
                        "multiply (hi / lo operand split): 4e-6 of the output maximum, inside the fp32 kernels' own tolerances")
    p.add_argument("--gpu_pipeline", type=str2bool, default=False,
                   help="keep the uint8 training images in HBM and crop/augment on the GPU (pesr_amd.input_pipeline)")
    p.add_argument("--lr_from_hr", type=str2bool, default=False,
                   help="build the training and validation sets from their HR/ folders alone: every HR image is cropped to multiples "
                        "of --scale and its LR image is made on the GPU by MATLAB-style bicubic resize (docs/modes.md section 4f)")
    p.add_argument("--degradation", type=str, default="bicubic", choices=["bicubic", "classical"],
                   help="how --lr_from_hr makes the LR images.  bicubic (default): the resize of section 4f.  classical: blind training "
                        "on LR = (HR blurred by a Gaussian kernel) subsampled, plus noise (docs/modes.md section 4j): every training "
                        "sample gets a kernel and a noise level of its own, made on the GPU each step; needs --lr_from_hr true "
                        "--gpu_pipeline true and no --synthetic")
    p.add_argument("--blur_sigma", type=str, default="",
                   help="with --degradation classical: LO,HI, the range of the Gaussian's standard deviation in HR pixels; default "
                        "0.2*scale,0.8*scale")
    p.add_argument("--blur_aniso", type=str2bool, default=False,
                   help="with --degradation classical: anisotropic kernels - a second sigma in [LO, the first] and an angle in [0, pi)")
    p.add_argument("--noise_sigma", type=float, default=0.0,
                   help="with --degradation classical: every sample gets noise of a standard deviation drawn from [0, this] grey levels; "
                        "0 (default) = no noise")
    p.add_argument("--jpeg_quality", type=str, default="",
                   help="with --degradation classical: LO,HI - every training sample's LR patch goes through a JPEG round trip on the GPU "
                        "at a quality drawn from LO .. HI (1 .. 100), after the noise and before the flips (docs/modes.md section 4l); "
                        "every validation image is compressed once at a quality of its own; needs --degradation classical "
                        "--lr_from_hr true --gpu_pipeline true; default: no compression")
    p.add_argument("--jpeg_chroma", type=str, default="420", choices=["420", "444"],
                   help="with --jpeg_quality: chroma at half resolution in both directions (420, default) or at full resolution (444)")
    p.add_argument("--resize_jitter", type=str, default="",
                   help="with --degradation classical: LO,HI (0.125 .. 8) - every training sample's LR patch is resized to r times its "
                        "sides, r drawn from [LO, HI], and back, each way with a filter drawn from bicubic, bilinear and box, on the GPU "
                        "(docs/modes.md section 4m); the noise then comes after the resize, the JPEG round trip last; every validation "
                        "image gets one such round trip of its own; needs --degradation classical --lr_from_hr true --gpu_pipeline true; "
                        "default: none")
    p.add_argument("--valid_ssim", type=str2bool, default=False,
                   help="validation also averages SSIM-Y (measured on the GPU, docs/modes.md section 4g) and prints it in a line of its "
                        "own; the best model is still chosen by PSNR")
    p.add_argument("--valid_shave", type=int, default=0,
                   help="drop a border of this many pixels before the validation PSNR (and SSIM, NIQE) is measured")
    p.add_argument("--valid_niqe", type=str, default="",
                   help="a NIQE pristine model (.npz from `python -m pesr_amd.niqe fit`, or the standard .mat): validation also averages "
                        "the NIQE of the results (measured on the GPU, docs/modes.md section 4k) and prints it in a line of its own; "
                        "the best model is still chosen by PSNR")
    p.add_argument("--valid_lpips", type=str, default="",
                   help="an LPIPS weight file (from `python -m pesr_amd.lpips pack`): validation also averages the LPIPS (v0.1, VGG variant, "
                        "measured on the GPU, docs/modes.md section 4n) of the results against the HR images and prints it in a line of "
                        "its own; the best model is still chosen by PSNR")
    p.add_argument("--valid_dists", type=str, default="",
                   help="a DISTS weight file (from `python -m pesr_amd.dists pack`): validation also averages the DISTS (measured on the "
                        "GPU, docs/modes.md section 4t) of the results against the HR images and prints it in a line of its own; the "
                        "best model is still chosen by PSNR")
    p.add_argument("--lpips_loss", type=str, default="",
                   help="an LPIPS weight file (from `python -m pesr_amd.lpips pack`) for --alpha_lpips: LPIPS (v0.1, VGG variant) of the "
                        "super-resolved batch against HR as a term of the generator's loss in --phase train (docs/modes.md section 4o)")
    p.add_argument("--alpha_lpips", type=float, default=0.0,
                   help="weight of the LPIPS term of the generator's loss; 0 (default) = off, and the step is then what it is without "
                        "the flag; > 0 needs --lpips_loss, --phase train and (--patch_size * --scale) % 16 == 0")
    p.add_argument("--alpha_ssim", type=float, default=0.0,
                   help="weight of the (1 - SSIM-Y) term of the generator's loss, in both phases (docs/modes.md section 4p: the SSIM of "
                        "--valid_ssim on the unquantised luma, differentiated on the GPU); 0 (default) = off, and the step is then what "
                        "it is without the flag; > 0 needs (--patch_size * --scale) >= 11")
    p.add_argument("--alpha_texture", type=float, default=0.0,
                   help="weight of the texture loss of the generator's loss (docs/modes.md section 4q: the distance between patch-wise "
                        "Gram matrices of relu1_1 / relu2_1 / relu3_1 of the VGG19 trunk that --alpha_vgg runs anyway); 0 (default) = "
                        "off, and the step is then what it is without the flag; > 0 needs --phase train")
    p.add_argument("--texture_patch", type=int, default=16,
                   help="side of the texture loss's patches, in each tap's own pixels (EnhanceNet: 16); it must divide the three tap "
                        "sizes (--patch_size * --scale, a half and a quarter of it); 0 = the whole map (Gatys / Johnson)")
    p.add_argument("--alpha_cx", type=float, default=0.0,
                   help="weight of the contextual loss of the generator's loss (docs/modes.md section 4r: -log CX of relu3_4 of the "
                        "VGG19 trunk that --alpha_vgg runs anyway); 0 (default) = off, and the step is then what it is without the "
                        "flag; > 0 needs --phase train and a (--patch_size * --scale) that is a multiple of 4 and at most 256")
    p.add_argument("--cx_h", type=float, default=0.5, help="bandwidth h of the contextual loss's weights exp((1 - d / (min d + 1e-5)) / h)")
    p.add_argument("--valid_tile", type=int, default=0,
                   help="validate every image as batches of overlapping tiles (docs/modes.md section 4h): the side of the square of LR "
                        "pixels a tile owns; 0 (default) = off, one Generator call on the whole image")
    p.add_argument("--valid_tile_halo", type=int, default=-1,
                   help="with --valid_tile: LR pixels of context around a tile; -1 = 2 * num_blocks + 4, the exact one")
    p.add_argument("--save_state_every", type=int, default=0,
                   help="at the end of every N-th epoch write <check_point>/<phase>/train_state.pt: both networks, both optimizers, the "
                        "schedulers, the epoch, the random streams (docs/modes.md section 4i); 0 (default) = never")
    p.add_argument("--resume", type=str, default="",
                   help="a training state file to continue from (with the epoch after the one it records), or 'auto': this run's own "
                        "<check_point>/<phase>/train_state.pt if it exists, a fresh start otherwise")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="keep an exponential moving average of the Generator's weights with this decay (typical: 0.999), updated inside "
                        "the Adam kernel; validation and the saved models then use the averaged weights.  0 (default) = off")
    return p


def device_lr_from_hr(scale, device):
    """The callable FolderSRDataset(lr_from_hr=...) wants, on the device resize: uint8 HWC array -> uint8 HWC array."""
    from pesr_amd.degrade import lr_image_u8
    return lambda hr: lr_image_u8(torch.from_numpy(np.array(hr)).to(device), scale).cpu().numpy()


VALID_DEGRADE_SEED = 20240229      # --degradation classical: the validation images' kernels and noise never change


def degradation_spec(args):
    """--degradation classical -> its DegradationSpec (None for bicubic); SystemExit naming the flags it needs.  No GPU is touched."""
    if args.jpeg_quality and not (args.degradation == "classical" and args.lr_from_hr and args.gpu_pipeline and not args.synthetic):
        raise SystemExit("train.py: --jpeg_quality compresses the LR patches the GPU makes from the HR pool: it needs --degradation classical "
                         "--lr_from_hr true --gpu_pipeline true and no --synthetic")
    if args.resize_jitter and not (args.degradation == "classical" and args.lr_from_hr and args.gpu_pipeline and not args.synthetic):
        raise SystemExit("train.py: --resize_jitter resizes the LR patches the GPU makes from the HR pool: it needs --degradation classical "
                         "--lr_from_hr true --gpu_pipeline true and no --synthetic")
    if args.degradation != "classical":
        return None
    if not (args.lr_from_hr and args.gpu_pipeline) or args.synthetic:
        raise SystemExit("train.py: --degradation classical makes every LR patch on the GPU from the HR pool: it needs --lr_from_hr true "
                         "--gpu_pipeline true and no --synthetic")
    from pesr_amd.degrade import DegradationSpec, parse_sigma_list
    lo, hi = parse_sigma_list(args.blur_sigma, "train.py", "--blur_sigma", (2,)) if args.blur_sigma else (0.2 * args.scale, 0.8 * args.scale)
    jlo = jhi = 0
    if args.jpeg_quality:
        from pesr_amd.jpeg import parse_quality
        jlo, jhi = parse_quality(args.jpeg_quality, "train.py", "--jpeg_quality", 2)
    rlo, rhi = parse_sigma_list(args.resize_jitter, "train.py", "--resize_jitter", (2,)) if args.resize_jitter else (0.0, 0.0)
    if args.resize_jitter and not 0.125 <= rlo <= rhi <= 8:      # (NaN too; check() alone would take 0,0 for "off")
        raise SystemExit(f"train.py: --resize_jitter {args.resize_jitter!r}: the range must be 0.125 <= LO <= HI <= 8")
    return DegradationSpec(lo, hi, bool(args.blur_aniso), float(args.noise_sigma), jlo, jhi, args.jpeg_chroma == "420", rlo, rhi).check(
        "train.py: --blur_sigma / --noise_sigma / --jpeg_quality / --resize_jitter")


def device_degrade_from_hr(scale, spec, device):
    """The callable FolderSRDataset(lr_from_hr=..., lr_from_hr_index=True) wants under --degradation classical: image i of the sorted
    folder is degraded whole, with parameters drawn from a stream that only VALID_DEGRADE_SEED and i decide - the validation PSNR
    is comparable across epochs and across a resume.  A spec with a resize jitter sends the image through the round trip of section
    4m (the noise then in its second resize), a spec with a JPEG range compresses it last (section 4l): both take their values from
    the same stream, after the other values."""
    import random
    from pesr_amd.degrade import gaussian_kernel, kernel_size, lr_image_u8
    K = kernel_size(scale, spec.sigma_hi)

    def make(hr, i):
        d = spec.named(spec.draw(random.Random(VALID_DEGRADE_SEED * 1000003 + i)))
        return lr_image_u8(torch.from_numpy(np.array(hr)).to(device), scale, gaussian_kernel(K, d["sigma1"], d["sigma2"], d["theta"]),
                           d["sigma_n"], d["q"], (d["jitter_r"], d["jitter_m1"], d["jitter_m2"]) if spec.jitter_hi else None,
                           d.get("jpeg_quality", 0), spec.jpeg_420).cpu().numpy()
    return make


def spawn_generator():
    """A generator of its own, started from torch's global stream (so torch.manual_seed still decides everything)."""
    g = torch.Generator()
    g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    return g


def make_loaders(args, rank, world, need_train=True, device=None):
    from data import FolderSRDataset, SyntheticSRDataset
    train_set = None
    # (the LR images are made here, in the parent process, before any loader worker is forked)
    from_hr = device_lr_from_hr(args.scale, device) if args.lr_from_hr and not args.synthetic else None
    spec = degradation_spec(args)
    if spec is not None:      # (the training set is the GPU loader's; this serves the validation set)
        from_hr = device_degrade_from_hr(args.scale, spec, device)
    if args.synthetic:
        train_set = SyntheticSRDataset(args.synthetic, args.patch_size, scale=args.scale)
        val_set = SyntheticSRDataset(min(args.num_valids, 2), args.patch_size, seed=99, scale=args.scale)
    else:
        if need_train:      # (the GPU input pipeline replaces the host training loader altogether)
            train_set = FolderSRDataset(os.path.join("data/origin/train", args.train_dataset), args.patch_size, args.num_repeats, True,
                                        scale=args.scale, lr_from_hr=from_hr)
        val_set = FolderSRDataset(os.path.join("data/origin/valid", args.valid_dataset), None, 1, False, fixed_length=10,
                                  scale=args.scale, lr_from_hr=from_hr, lr_from_hr_index=spec is not None)
    sampler = train_loader = None
    if train_set is not None:
        sampler = DistributedSampler(train_set, world, rank, shuffle=True, drop_last=True) if world > 1 else None
        # The shuffle (one GPU; DistributedSampler's is a function of the epoch) and the seed of the loader's workers are drawn from
        # generators of their own.  The iterator draws its workers' seed when it is CREATED - in the first epoch of a process, not in
        # the later ones, which reuse the workers -, so on torch's global stream a resumed run would be one draw ahead of the run that
        # was never stopped.  The shuffle generator is part of the training state (main: checkpoint.rng_snapshot).
        train_loader = DataLoader(train_set, batch_size=args.batch_size // world,
                                  sampler=sampler if sampler is not None else RandomSampler(train_set, generator=spawn_generator()),
                                  generator=spawn_generator(),
                                  num_workers=4, pin_memory=True, drop_last=True, persistent_workers=True)   # (forked once: a fork of a
        # process with a GPU context's mappings takes seconds, and without this flag every epoch forks its four workers anew)
    val_loader = DataLoader(val_set, batch_size=1, shuffle=False, num_workers=1, pin_memory=True)
    return train_loader, val_loader, sampler


class GpuLoader:
    """Iterable with the DataLoader's contract (yields (lr, hr) batches) on top of GpuPatchSampler, with the reference's epoch
    composition (reference data.py:60-77 + DataLoader(shuffle=True, drop_last=True), train.py:96-97): every image appears
    exactly num_repeats times per epoch in a fresh random order; under torch.distributed the epoch's permutation (seeded by
    the epoch, identical on all ranks) is dealt round-robin to the ranks like DistributedSampler does, so no image is drawn
    twice into one global batch position and every sample is seen by exactly one rank."""

    def __init__(self, sampler, batch, patch, n_images, num_repeats, rank, world, seed=1):
        import random
        self.sampler, self.batch, self.patch = sampler, batch, patch
        self.n, self.rep, self.rank, self.world, self.seed = n_images, num_repeats, rank, world, seed
        self.epoch = 0
        self.rng = random.Random(seed * 7919 + rank)          # crop origins / augmentation: per-rank stream

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return (self.n * self.rep) // (self.batch * self.world)

    def epoch_indices(self):
        import random
        order = list(range(self.n)) * self.rep
        random.Random(self.seed * 1000003 + self.epoch).shuffle(order)
        usable = len(self) * self.batch * self.world            # drop_last
        return order[self.rank:usable:self.world]

    def __iter__(self):
        idx = self.epoch_indices()
        for b in range(len(self)):
            picks = self.sampler.draw_for(idx[b * self.batch:(b + 1) * self.batch], self.patch, self.rng, augment=True)
            yield self.sampler.assemble(picks, self.patch, nhwc=True)


def make_gpu_loader(args, rank, world, device):
    import glob
    from PIL import Image
    from pesr_amd.input_pipeline import GpuPatchSampler
    root = os.path.join("data/origin/train", args.train_dataset)
    if args.lr_from_hr:
        hrs = [np.asarray(Image.open(p).convert("RGB")) for p in sorted(glob.glob(os.path.join(root, "HR", "*.png")))]
        return GpuLoader(GpuPatchSampler.from_hr(hrs, device, scale=args.scale, degradation=degradation_spec(args)), args.batch_size // world, args.patch_size, len(hrs),
                         args.num_repeats, rank, world)
    lr_paths = sorted(glob.glob(os.path.join(root, "LR", "*.png")))
    lrs = [np.asarray(Image.open(p).convert("RGB")) for p in lr_paths]
    hrs = [np.asarray(Image.open(os.path.join(root, "HR", os.path.basename(p))).convert("RGB")) for p in lr_paths]
    return GpuLoader(GpuPatchSampler(lrs, hrs, device, scale=args.scale), args.batch_size // world, args.patch_size, len(lrs), args.num_repeats,
                     rank, world)


def build_vgg(args, device, rank, world):
    """The reference's perceptual loss uses torchvision's PRETRAINED vgg19 (reference model/vgg.py:8); training against anything
    else silently produces a different model.  Order of preference: --vgg_weights file; torchvision's own pretrained weights if
    that package is importable; else refuse, unless --synthetic / --allow_random_vgg ask for seeded random features - which are
    then made identical on every rank (seeded construction + broadcast from rank 0), so all replicas optimise the same loss."""
    import warnings
    from model import VGG
    if args.vgg_weights:
        return VGG(args.vgg_weights).to(device)
    # Only "the package or its model-zoo file is not there" counts as unavailable (ImportError; URLError / OSError of the
    # download); anything else - a corrupt cache, out of memory - is an error, not a reason to train on random features.
    import urllib.error
    sd, why = None, ""
    try:
        import torchvision
        sd = torchvision.models.vgg19(pretrained=True).state_dict()
    except (ImportError, urllib.error.URLError, OSError) as e:
        why = type(e).__name__
    if world > 1:
        # every rank must take the same branch: the pretrained weights are used only if ALL ranks have them
        ok = torch.tensor([1 if sd is not None else 0], device=device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            sd = None
    if sd is not None:
        import tempfile
        with tempfile.NamedTemporaryFile(suffix=".pt") as f:
            torch.save(sd, f.name)
            return VGG(f.name).to(device)
    if not (args.synthetic or args.allow_random_vgg):
        raise SystemExit("train.py: the GAN phase needs torchvision's pretrained vgg19 weights (reference model/vgg.py:8): pass "
                         "--vgg_weights <state_dict file>, or --allow_random_vgg true for a run whose perceptual loss is NOT the "
                         f"reference's (torchvision's weights unavailable on at least one rank: {why or 'another rank'})")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        state = torch.random.get_rng_state()
        torch.manual_seed(20180917)
        vgg = VGG().to(device)
        torch.random.set_rng_state(state)
    if world > 1:
        for p in vgg.parameters():
            dist.broadcast(p.data, 0)
    if rank == 0:
        print("WARNING: VGG19 features are RANDOM (seeded): the perceptual loss of this run is not the reference's")
    return vgg


def attention_of(args):
    """--attention / --ca_reduction -> the reduction of the Generator's channel attention (0: none); SystemExit naming the flag.  No GPU
    is touched."""
    if args.ca_reduction < 1:
        raise SystemExit(f"train.py: --ca_reduction {args.ca_reduction} must be at least 1")
    # (the default 16 is not held against a run without attention whose width it does not divide)
    if args.num_channels % args.ca_reduction and (args.attention == "ca" or args.ca_reduction != 16):
        raise SystemExit(f"train.py: --ca_reduction {args.ca_reduction} does not divide --num_channels {args.num_channels}")
    if args.attention == "none":
        return 0
    if args.num_channels % 4 or args.num_channels > 2048:
        raise SystemExit(f"train.py: --attention ca needs --num_channels to be a multiple of 4 up to 2048, got {args.num_channels}")
    return args.ca_reduction


def d_arch_of(args):
    """--d_arch / --d_width -> "vgg" or "unet"; SystemExit naming the flag.  No GPU is touched."""
    if args.d_width < 16 or args.d_width % 16:
        raise SystemExit(f"train.py: --d_width {args.d_width} must be a positive multiple of 16")
    if args.d_arch == "unet" and args.GP and args.phase != "pretrain":      # (the pretrain phase builds no Discriminator at all)
        raise SystemExit("train.py: --GP true with --d_arch unet is not built: the gradient penalty needs a twice-differentiable "
                         "bilinear upsample node (docs/modes.md section 4v); use --d_arch vgg or --GP false")
    side = args.patch_size * args.scale
    if args.d_arch == "unet" and args.phase != "pretrain" and (side < 8 or side % 8):
        raise SystemExit(f"train.py: --d_arch unet needs (--patch_size * --scale) to be a multiple of 8, here {args.patch_size} * "
                         f"{args.scale} = {side} (three stride-2 stages and their x2 upsamplings)")
    return args.d_arch


def wattn_of(args):
    """--wattn_every / --wattn_dim -> (E, D) of the Generator's window-attention blocks, (0, 0) for none; SystemExit naming the flag.
    No GPU is touched."""
    from pesr_amd import ops as _ops
    if args.wattn_every < 0:
        raise SystemExit(f"train.py: --wattn_every {args.wattn_every} must be 0 (off) or positive")
    if args.wattn_dim < 0:
        raise SystemExit(f"train.py: --wattn_dim {args.wattn_dim} must be 0 (--num_channels / 2) or a positive multiple of 32")
    if args.wattn_every == 0:
        return 0, 0
    if args.wattn_every > args.num_blocks:
        raise SystemExit(f"train.py: --wattn_every {args.wattn_every} is above --num_blocks {args.num_blocks}: it would add no block")
    dim = args.wattn_dim or args.num_channels // 2
    try:
        _ops.wattn_check_widths("train.py", args.num_channels, dim)
    except ValueError as e:
        flag = "--num_channels" if str(e).startswith("train.py: n_feats") else "--wattn_dim" + ("" if args.wattn_dim else " (0: --num_channels / 2)")
        raise SystemExit(f"train.py: {flag} with --wattn_every {args.wattn_every}: {e}")
    return args.wattn_every, dim


def wattn_norm_of(args):
    """--wattn_norm -> 'ln' or None; SystemExit naming the flag where there is no block to normalise.  No GPU is touched."""
    if args.wattn_norm == "ln" and args.wattn_every <= 0:
        raise SystemExit("train.py: --wattn_norm ln needs --wattn_every E > 0: without window-attention blocks there is nothing to normalise")
    return "ln" if args.wattn_norm == "ln" else None


def check_pretrained_wattn_norm(sd, args, path):
    """A --pretrained_model whose window-attention blocks have (or lack) the LayerNorm this run lacks (or has): SystemExit naming both."""
    from pesr_amd.model import wattn_norm_of_state_dict
    try:
        found = wattn_norm_of_state_dict(sd)
    except ValueError as e:
        raise SystemExit(f"train.py: --pretrained_model {path}: {e}")
    if found != args.wattn_norm:
        raise SystemExit(f"train.py: --pretrained_model {path} has window-attention blocks with norm '{found}', this run has "
                         f"--wattn_norm {args.wattn_norm}")
    return sd


def check_pretrained_wattn(sd, args, path):
    """A --pretrained_model whose window-attention blocks are not this run's: SystemExit naming both."""
    from pesr_amd.model import wattn_of_state_dict
    from pesr_amd.model.pesr import wattn_positions
    try:
        found = wattn_of_state_dict(sd)
    except ValueError as e:
        raise SystemExit(f"train.py: --pretrained_model {path}: {e}")
    every, dim = wattn_of(args)
    mine = (wattn_positions(every, args.num_blocks), dim)
    if found != mine:
        say = lambda w: f"window-attention blocks of width {w[1]} after the residual blocks {list(w[0])}" if w[0] else \
            "no window-attention blocks"
        raise SystemExit(f"train.py: --pretrained_model {path} has {say(found)}, this run (--wattn_every {args.wattn_every} --wattn_dim "
                         f"{args.wattn_dim}) has {say(mine)}")
    return sd


def check_pretrained_attention(sd, args, path):
    """A --pretrained_model whose channel attention is not this run's: SystemExit naming both (instead of load_state_dict's key dump)."""
    from pesr_amd.model import attention_of_state_dict
    try:
        found = attention_of_state_dict(sd)
    except ValueError as e:
        raise SystemExit(f"train.py: --pretrained_model {path}: {e}")
    mine = attention_of(args)
    if found != mine:
        say = lambda r: f"--attention ca --ca_reduction {r}" if r else "--attention none"
        raise SystemExit(f"train.py: --pretrained_model {path} was trained with {say(found)}, this run has {say(mine)}")
    return sd


def check_limits(args, world):
    """Shape limits of the HIP path, checked up front with a clear message instead of a PESR_EINVAL deep inside a step."""
    if args.batch_size % world:
        raise SystemExit(f"train.py: --batch_size {args.batch_size} must be a multiple of the {world} ranks")
    if args.scale not in (2, 3, 4):
        raise SystemExit(f"train.py: --scale {args.scale} is not supported; the upsamplers are x2, x3 and x4")
    if args.scale != 4 and args.precision != "fp32":
        raise SystemExit(f"train.py: --precision {args.precision} is checked for --scale 4 only; use --precision fp32 with --scale "
                         f"{args.scale}")
    from pesr_amd.tile import check_flags
    check_flags("train.py", ("--valid_tile", "--valid_tile_halo"), args.valid_tile, args.valid_tile_halo, 1, args.num_blocks, args.scale)
    if not 0.0 <= args.ema_decay < 1.0:
        raise SystemExit(f"train.py: --ema_decay {args.ema_decay} must be 0 (off) or inside (0, 1)")
    if args.save_state_every < 0:
        raise SystemExit(f"train.py: --save_state_every {args.save_state_every} must be 0 (never) or a number of epochs")
    if args.phase != "pretrain" and args.scale == 4 and args.patch_size % 4:
        raise SystemExit("train.py: the GAN phase needs --patch_size % 4 == 0 (HR patches must survive four stride-2 stages and "
                         "VGG's four 2x2 max-pools, which this implementation does for even sizes only)")
    if args.phase != "pretrain" and (args.patch_size * args.scale) % 16:
        raise SystemExit(f"train.py: the GAN phase needs (--patch_size * --scale) % 16 == 0, here {args.patch_size} * {args.scale} = "
                         f"{args.patch_size * args.scale} (HR patches must survive four stride-2 stages and VGG's four 2x2 max-pools, "
                         "which this implementation does for even sizes only)")


def scorer_of(args):
    """The --valid_* flags -> the Scorer of the validation (pesr_amd/quality.py); SystemExit naming the flags.  No GPU is touched."""
    from pesr_amd.quality import Scorer
    scorer = Scorer("train.py", args.valid_ssim, args.valid_shave, args.valid_niqe, args.valid_lpips,
                    flags=("--valid_niqe", "--valid_lpips", "--valid_shave"), size_flags="--valid_shave / --patch_size",
                    dists=args.valid_dists, dists_flag="--valid_dists")
    if args.synthetic:          # (the synthetic validation images are patch-sized; a folder's sizes are known when it is read)
        scorer.check_size(args.patch_size * args.scale, args.patch_size * args.scale, "the synthetic validation images")
    return scorer


def lpips_model_of(args):
    """--valid_lpips -> its model (None without the flag), as scorer_of(args) holds it."""
    return scorer_of(args).lpips_model


def loss_terms_of(args, valid_lpips_model=None):
    """The flags of the optional terms of the generator's loss (pesr_amd/loss_terms.py TERMS) -> their keyword arguments for Trainer;
    SystemExit naming the flags.  Per term, in table order: the weight rule; the term's own parameters; off: nothing else; the phase;
    the side of the HR patches.  valid_lpips_model: the model --valid_lpips loaded, for the term that can share it.  No GPU is touched."""
    from pesr_amd.loss_terms import TERMS
    side, kw = args.patch_size * args.scale, {}
    what = f"(--patch_size * --scale) = {args.patch_size} * {args.scale} = {side}"
    for cls in TERMS:
        alpha = getattr(args, cls.weight)
        if not alpha >= 0:
            raise SystemExit(f"train.py: {cls.flag} {alpha} must be >= 0 (0 = off)")
        mine = cls.from_flags(args, "train.py", valid_lpips_model)
        try:
            term = cls(**mine)
        except ValueError as e:         # (the text begins with the parameter's name, which is its flag's)
            raise SystemExit(f"train.py: {cls.flag} {alpha}: --{e}")
        kw.update(mine)
        if not term.on:
            continue
        if args.phase not in term.phases:
            raise SystemExit("train.py: " + term.wrong_phase(args.phase))
        why = term.check(side, what)
        if why:
            raise SystemExit("train.py: " + why)
    return kw


def main(argv=None):
    args = build_parser().parse_args(argv)
    degradation_spec(args)      # (refuses a classical run without its companion flags before anything else starts)
    attention = attention_of(args)
    wattn_every, wattn_dim = wattn_of(args)
    wattn_norm = wattn_norm_of(args)
    d_arch = d_arch_of(args)
    scorer = scorer_of(args)
    loss_terms = loss_terms_of(args, scorer.lpips_model)
    world =int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # TEST HOOK (tests/test_dp_gpu.py): PESR_DP_SHARE_GPU=1 + PESR_DP_BACKEND=gloo lets the ranks time-share cuda:0 over gloo, so
    # that the multi-rank branches of this script run on a one-GPU box
    backend = os.environ.get("PESR_DP_BACKEND", "nccl")
    if os.environ.get("PESR_DP_SHARE_GPU") == "1":
        assert backend == "gloo", "RCCL refuses two ranks on one device"
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    check_limits(args, world)
    if rank == 0:
        print("_____________YOUR SETTINGS_____________")
        for k, v in vars(args).items():
            print("%20s: %s" % (k, v))

    from model import Discriminator, Generator, VGG
    from pesr_amd import ops as _ops
    _ops.set_precision(args.precision)
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    from pesr_amd.quality import ScoreError
    from pesr_amd.tile import describe, receptive_halo, tiled_forward
    valid_halo = receptive_halo(args.num_blocks, args.scale) if args.valid_tile_halo == -1 else args.valid_tile_halo
    if args.valid_tile and rank == 0:
        print(describe(args.valid_tile, valid_halo, receptive_halo(args.num_blocks, args.scale), attention=bool(attention),
                       wattn=bool(wattn_every)))

    gpu_pipe = args.gpu_pipeline and not args.synthetic
    train_loader, val_loader, sampler = make_loaders(args, rank, world, need_train=not gpu_pipe, device=device)
    if gpu_pipe:
        train_loader = sampler = make_gpu_loader(args, rank, world, device)      # (it has set_epoch like a DistributedSampler)
    opt = {"patch_size": args.patch_size, "num_channels": args.num_channels, "depth": args.num_blocks,
           "res_scale": args.res_scale, "spectral_norm": args.spectral_norm, "scale": args.scale}
    if attention:
        opt.update(attention="ca", ca_reduction=attention)
    if wattn_every:
        opt.update(wattn_every=wattn_every, wattn_dim=wattn_dim)
    if wattn_norm:
        opt.update(wattn_norm=wattn_norm)
    from pesr_amd import checkpoint
    resume_path = checkpoint.resolve_resume(args.resume, args.check_point, args.phase)
    state = None
    if resume_path is not None:
        state = checkpoint.load_state(resume_path)          # (every rank reads the file)
        checkpoint.check_flags(state, args, resume_path)
    elif args.resume and rank == 0:
        print("resume: no %s yet, starting fresh" % checkpoint.state_path(args.check_point, args.phase))
    G = Generator(opt)
    if args.pretrained_model and state is None:
        sd = check_pretrained_attention(torch.load(args.pretrained_model, map_location="cpu"), args, args.pretrained_model)
        G.load_state_dict(check_pretrained_wattn_norm(check_pretrained_wattn(sd, args, args.pretrained_model), args, args.pretrained_model))
    G = G.to(device)
    gan = args.phase != "pretrain"
    from model import build_discriminator
    D = build_discriminator(dict(opt, d_width=args.d_width) if d_arch == "unet" else opt, d_arch).to(device) if gan else None
    vgg = build_vgg(args, device, rank, world) if gan else None

    optim_G = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=args.learning_rate, betas=(0.9, 0.999),
                       ema_decay=args.ema_decay)
    optim_D = FlatAdam(D.parameters(), lr=args.learning_rate, betas=(0.9, 0.999)) if gan else None
    if world > 1:  # replicas start identical
        dist.broadcast(optim_G.flat.flat_p, 0)
        if optim_G.flat_ema is not None:
            optim_G.flat_ema.copy_(optim_G.flat.flat_p)      # (the average starts from the weights every replica now holds)
        if gan:
            dist.broadcast(optim_D.flat.flat_p, 0)
    scheduler_G = lr_scheduler.StepLR(optim_G, step_size=args.lr_step, gamma=0.5)
    scheduler_D = lr_scheduler.StepLR(optim_D, step_size=args.lr_step, gamma=0.5) if gan else None
    trainer = Trainer(G, D, vgg, optim_G, optim_D, gan_type=args.gan_type, focal_loss=args.focal_loss, fl_gamma=args.fl_gamma,
                      alpha_vgg=args.alpha_vgg, alpha_gan=args.alpha_gan, alpha_tv=args.alpha_tv, alpha_l1=args.alpha_l1,
                      world_size=world, gradient_penalty=args.GP, **loss_terms)

    check_point = os.path.join(args.check_point, args.phase)
    # what checkpoint.rng_snapshot / rng_restore get besides the process-wide streams: the GPU input pipeline's crop stream, or the
    # host loader's shuffle generator (one GPU)
    rng_extra = {"gpu_loader": train_loader} if gpu_pipe else {"shuffle": getattr(train_loader.sampler, "generator", None)}
    tb = None
    if rank == 0:
        os.makedirs(check_point, exist_ok=True)
        try:
            from tensorboardX import SummaryWriter
            tb = SummaryWriter(check_point)
        except ImportError:
            pass
    best_psnr = 0.0
    first_epoch = 1
    if state is not None:
        checkpoint.restore(state, G, D, optim_G, optim_D, scheduler_G, scheduler_D)
        best_psnr, first_epoch = state["best_psnr"], state["epoch"] + 1
        if rank == 0:
            print("resume: %s, epoch %d done, going on with epoch %d at lr %g (--pretrained_model, --learning_rate and --lr_step are "
                  "the state's)" % (resume_path, state["epoch"], first_epoch, optim_G.param_groups[0]["lr"]))
            if state["world"] != world:
                print("resume: the state was saved by %d rank(s), this run has %d: model, optimizer and schedule state are exact, the "
                      "random streams start fresh" % (state["world"], world))
    # with --ema_decay the averaged weights are what is validated and saved (the raw ones live in the state file)
    G_eval = optim_G.ema_module(G) if args.ema_decay > 0 else G
    ema_tag = " (EMA)" if args.ema_decay > 0 else ""
    keys = (("l1", "vgg", "g", "tv", "d") if gan else ("l1",)) + tuple(t.key for t in trainer.terms)
    graphed, graph_shapes, eager_at_shape = None, None, 0
    use_graph = device.type == "cuda" and (world == 1 if args.hip_graph == "auto" else str2bool(args.hip_graph))
    # data-parallel schedule: fixed by flag, or measured once (inside the first epoch that is long enough for it)
    dp_on = optim_G.buckets.enabled
    dp_calibrate = dp_on and args.dp_policy == "auto"
    if dp_on and args.dp_policy != "auto":
        trainer.set_dp_policy(args.dp_policy)
    elif dp_calibrate and state is not None and state["world"] == world and state["dp"]["policy"] is not None:
        # the first run measured (and its measurement consumed training steps): a resumed run takes that schedule, it does not re-time
        dp_calibrate = False
        trainer.set_dp_policy(state["dp"]["policy"])
        use_graph = use_graph or bool(state["dp"].get("graph"))
        if rank == 0:
            now = [type(t).__name__ for t in trainer._transports()]
            print("data-parallel schedule: '%s' as recorded in the state (not measured again)%s" % (
                trainer.dp_policy, "" if not now or now[0] == state["dp"]["transport"] else
                "; gradient exchange over %s, the state's run used %s" % (now[0], state["dp"]["transport"])))
    CALIB_STEPS = 3
    peer_cand = str2bool(args.dp_peer_candidate) and world > 1
    # iterations the calibration consumes at most (its own worst-case count: eager candidates, the peer-memory candidate, the capture's
    # batch and the replays - ADVICE r05: the peer candidate was not counted and the calibration could run off the end of an epoch)
    calib_need = Trainer.calibration_batches("gan" if gan else "pretrain", CALIB_STEPS, graph=args.hip_graph == "auto", peer_candidate=peer_cand) + 2

    if state is not None and state["world"] == world:
        # last of all: nothing between here and the first batch draws from these streams
        checkpoint.rng_restore(state["rng"][rank], device, **rng_extra)
    state = None        # (its tensors are loaded; drop the host copy)
    for epoch in range(1, args.num_epochs + 1):
        if epoch < first_epoch:     # --resume: the state holds these epochs
            continue
        # The reference calls scheduler.step() at epoch START (train.py:156,185-186); under its pinned torch 0.4 the
        # constructor leaves last_epoch = -1, so epoch e trains at lr*0.5^((e-1)//lr_step) (first halving: epoch lr_step+1).
        # On torch >= 1.1 the constructor already counts one step, so the same schedule is: step at the END of every epoch.
        cur_lr = optim_G.param_groups[0]["lr"]
        if sampler is not None:
            sampler.set_epoch(epoch)
        running = torch.zeros(len(keys), device=device)      # accumulated on the device: one host sync per epoch
        iters = 0
        batch_iter = iter(train_loader)
        n_iters = len(train_loader) if not args.max_iters else min(len(train_loader), args.max_iters)
        consumed = [0]

        def next_batch():
            a, b = next(batch_iter)
            consumed[0] += 1
            return a.to(device, non_blocking=True), b.to(device, non_blocking=True)

        while consumed[0] < n_iters:
            try:
                lr_img, hr_img = next_batch()
            except StopIteration:
                break
            if graphed is not None and lr_img.shape == graph_shapes[0] and hr_img.shape == graph_shapes[1]:
                logs = graphed(lr_img, hr_img)
            else:
                logs = trainer.gan_step(lr_img, hr_img) if gan else trainer.pretrain_step(lr_img, hr_img)
                if dp_calibrate and iters >= 1 and n_iters - consumed[0] >= calib_need:
                    # every rank is at the same iteration of equally long loaders: the calibration's collectives line up.  Its
                    # steps are real training steps (their losses are not added to this epoch's averages).
                    info = trainer.calibrate_dp_policy("gan" if gan else "pretrain", next_batch, steps=CALIB_STEPS, peer_candidate=peer_cand,
                                                       graph=args.hip_graph == "auto",
                                                       will_capture=args.hip_graph != "auto" and str2bool(args.hip_graph))
                    dp_calibrate = False
                    if rank == 0:
                        print("data-parallel schedule:", info)
                        # a run is reproduced bit for bit with an explicit --dp_policy (the bucket schedule decides RCCL's
                        # reduction order): the choice is kept next to the checkpoints
                        with open(os.path.join(check_point, "dp_policy.json"), "w") as fh:
                            json.dump({"dp_policy": trainer.dp_policy, **info}, fh, indent=1)
                    if info["chosen"].startswith("graph"):
                        graphed, graph_shapes = trainer.dp_step, (lr_img.shape, hr_img.shape)
                    # (--hip_graph true / false: the flag decides and only the bucket schedule was measured; the capture below
                    # then runs with that schedule)
                if use_graph and graphed is None and not dp_calibrate:
                    # capture after TWO eager steps at these shapes: the second one has seen every weight packing the first one
                    # created (some only in its backward pass), so nothing is allocated or uploaded under capture
                    shapes = (lr_img.shape, hr_img.shape)
                    eager_at_shape = eager_at_shape + 1 if shapes == graph_shapes else 1
                    graph_shapes = shapes
                    if eager_at_shape >= 2:
                        graphed = (trainer.capture_gan_step if gan else trainer.capture_pretrain_step)(lr_img, hr_img)
            running += torch.stack([logs[k].float() for k in keys])
            iters += 1
        if dp_calibrate:
            # No epoch will get longer: with too few iterations left behind the second step for the measurement (short epochs
            # or a small --max_iters) the schedule stays the default one - said once, and --hip_graph true can capture now.
            dp_calibrate = False
            if rank == 0:
                print("data-parallel schedule: an epoch has %d iterations, the measurement needs %d behind the second one - keeping "
                      "'%s' (choose with --dp_policy)" % (n_iters, calib_need, trainer.dp_policy))
        if world > 1:
            dist.all_reduce(running)
            running /= world
            if gan:  # the TV term is a sum over the global batch
                running[keys.index("tv")] *= world
        avg = (running / max(iters, 1)).tolist()
        if rank == 0:
            print("Epoch [%d/%d] lr %g  " % (epoch, args.num_epochs, cur_lr) + "  ".join("%s %.4f" % kv for kv in zip(keys, avg)))
            if tb is not None:
                tb.add_scalar("Learning rate", cur_lr, epoch)
                names = {"l1": "L1 Loss", "vgg": "VGG Loss", "g": "G Loss", "tv": "TV Loss", "d": "D Loss",
                         **{t.key: t.title for t in trainer.terms}}
                for k, v in zip(keys, avg):
                    tb.add_scalar(names[k] if gan or k != "l1" else "Pretrain Loss", v, epoch)

        # validation on rank 0 (full images, batch 1, no_grad), reference train.py:281-295
        if rank == 0:
            scores = []
            if G_eval is not G:
                optim_G.refresh_ema()       # the steps of this epoch rewrote the averaged weights through raw pointers
            with torch.no_grad():
                for lr_img, hr_img in val_loader:
                    if args.valid_tile:
                        sr, _ = tiled_forward(G_eval, lr_img.to(device), args.scale, args.valid_tile, valid_halo)
                    else:
                        sr = G_eval(lr_img.to(device))
                    try:
                        scores.append(scorer.score(sr, hr_img.to(device)))
                    except ScoreError as e:
                        raise SystemExit(f"train.py: {e.flags}: a validation image: {e}")
            means = scorer.mean(scores, scorer.columns())
            val_psnr = means["PSNR-Y"]
            # per column: "Finish valid [e/E]. NAME: value" and the tensorboard scalar "Validate NAME"
            for line, tag, value in scorer.valid_lines(epoch, args.num_epochs, means, ema_tag):
                print(line)
                if tb is not None:
                    tb.add_scalar(tag, value, epoch)
            if not gan and val_psnr > best_psnr:
                best_psnr = val_psnr
                torch.save(G_eval.state_dict(), os.path.join(check_point, "best_model.pt"))
            elif gan and epoch % args.snapshot_every == 0:
                torch.save(G_eval.state_dict(), os.path.join(check_point, "model_%d.pt" % epoch))
        scheduler_G.step()
        if gan:
            scheduler_D.step()
        if args.save_state_every and epoch % args.save_state_every == 0:
            # after validation and the scheduler steps: the file describes the run as epoch + 1 will find it
            rngs = checkpoint.gather_rng(checkpoint.rng_snapshot(device, **rng_extra), rank, world)
            if rank == 0:
                st = checkpoint.build_state(args, epoch, best_psnr, G, D, optim_G, optim_D, scheduler_G, scheduler_D, trainer, world, rngs)
                st["dp"]["graph"] = graphed is not None
                checkpoint.atomic_save(st, checkpoint.state_path(args.check_point, args.phase))
        if world > 1:
            dist.barrier()
    if world > 1:
        from pesr_amd import comm
        comm.close_transports()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
