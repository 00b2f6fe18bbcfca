"""Image <-> tensor helpers, the Y-channel PSNR of the reference (reference utils.py:10-41), the Y-channel SSIM beside it
(docs/modes.md section 4g) and the no-reference NIQE (section 4k), device-agnostic, and the full-reference LPIPS (section 4n) and
DISTS (section 4t), which run on the GPU only.

Tensors carry raw 0..255 values (no /255 anywhere).  Metrics run in numpy on the host exactly as the
reference does; nothing here is on the hot path.
"""
import os
import shutil

import numpy as np
import torch

_Y_COEF = np.array([65.738, 129.057, 25.064]) / 256.0


def default_device():
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def rgb2y(rgb):
    """ITU-R BT.601 luma of an HWC RGB array, offset 16 (reference utils.py:10-11)."""
    return np.dot(rgb[..., :3], _Y_COEF) + 16


def tensors_to_imgs(tensors):
    """[1,3,H,W] float tensors -> uint8 HWC arrays: clip to 0..255, round half-to-even, cast (reference utils.py:13-18)."""
    out = []
    for t in tensors:
        a = t.detach().squeeze(0).float().cpu().numpy()
        out.append(np.clip(a, 0, 255).round().transpose(1, 2, 0).astype(np.uint8))
    return out


def imgs_to_tensors(imgs, device=None):
    """uint8 HWC arrays -> [1,3,H,W] float tensors on `device` (reference utils.py:20-25 hard-codes .cuda())."""
    device = default_device() if device is None else device
    return [torch.from_numpy(np.ascontiguousarray(i.transpose(2, 0, 1))[None].astype(np.float32)).to(device) for i in imgs]


def normalize(tensors):
    return [t.clamp(0, 255) / 255 for t in tensors]


def _shaved(t, shave):
    shave = int(shave)
    if shave < 0 or 2 * shave >= min(t.shape[-2], t.shape[-1]):
        raise ValueError(f"shave {shave} leaves nothing of a {t.shape[-2]} x {t.shape[-1]} image")
    return t[..., shave:t.shape[-2] - shave, shave:t.shape[-1] - shave]


def compute_PSNR(out, lbl, shave=0):
    """PSNR on the rounded Y channel of two [1,3,H,W] tensors (reference utils.py:32-41).  GPU tensors are measured on the
    device (pesr_amd.ops.psnr_y, bit-identical: integer-valued terms in double); only the scalar comes back.  shave > 0 drops a
    border of that many pixels from both images first (the convention of the super-resolution tables: shave = scale)."""
    if shave:
        out, lbl = _shaved(out, shave), _shaved(lbl, shave)
    if torch.is_tensor(out) and torch.is_tensor(lbl) and out.is_cuda and lbl.is_cuda and out.dtype == torch.float32 \
            and lbl.dtype == torch.float32 and out.dim() == 4 and out.shape[0] == 1 and out.shape == lbl.shape:
        from pesr_amd import ops
        return float(ops.psnr_y(out.detach(), lbl.detach())[1])
    o, l = tensors_to_imgs([out, lbl])
    yo = np.clip(rgb2y(o), 0, 255).round()
    yl = np.clip(rgb2y(l), 0, 255).round()
    rmse = np.sqrt(np.mean((yo - yl) ** 2))
    return 20 * np.log10(255 / rmse)


def _ssim_luma(t):
    """[1,3,H,W] or [3,H,W] tensor / array -> the integer-valued float64 Y image of the PSNR-Y, [H, W]."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"compute_SSIM: expected a [1, 3, H, W] or [3, H, W] image, got {tuple(a.shape)}")
    rgb = np.rint(np.clip(a.astype(np.float64), 0.0, 255.0))
    y = ((rgb[0] * _Y_COEF[0] + rgb[1] * _Y_COEF[1]) + rgb[2] * _Y_COEF[2]) + 16.0
    return np.rint(np.clip(y, 0.0, 255.0))


def _ssim_filter(v, g):
    """[M, H, W] -> [M, H-10, W-10]: the 11-tap window along the height, then along the width, "valid" region, taps ascending."""
    ho, wo = v.shape[1] - 10, v.shape[2] - 10
    acc = np.zeros((v.shape[0], ho, v.shape[2]))
    for k in range(11):
        acc = acc + g[k] * v[:, k:k + ho, :]
    out = np.zeros((v.shape[0], ho, wo))
    for k in range(11):
        out = out + g[k] * acc[:, :, k:k + wo]
    return out


def compute_SSIM(out, lbl, shave=0):
    """SSIM on the rounded Y channel of two images (docs/modes.md section 4g): Wang et al.'s ssim_index.m as the super-resolution
    tables use it - 11 x 11 Gaussian window of sigma 1.5, "valid" region, K1 = 0.01, K2 = 0.03, L = 255, a border of `shave`
    pixels dropped first.  float32 GPU tensors [N,3,H,W] are measured on the device (pesr_amd.ops.ssim_y; the mean over the N pairs
    comes back); anything else ([1,3,H,W] / [3,H,W] tensors or arrays) goes through numpy in float64 with the same definition.
    ValueError when the shaved image is smaller than the window or the shapes differ."""
    shave = int(shave)
    if shave < 0:
        raise ValueError(f"compute_SSIM: shave must be >= 0, got {shave}")
    if tuple(out.shape) != tuple(lbl.shape):
        raise ValueError(f"compute_SSIM: the two images differ in shape: {tuple(out.shape)} and {tuple(lbl.shape)}")
    if min(out.shape[-2], out.shape[-1]) - 2 * shave < 11:
        raise ValueError(f"compute_SSIM: a {out.shape[-2]} x {out.shape[-1]} image with shave {shave} leaves less than the 11 x 11 "
                         "window")
    if torch.is_tensor(out) and torch.is_tensor(lbl) and out.is_cuda and lbl.is_cuda and out.dtype == torch.float32 \
            and lbl.dtype == torch.float32 and out.dim() == 4 and out.shape[1] == 3:
        from pesr_amd import ops
        return float(ops.ssim_y(out.detach(), lbl.detach(), shave).mean())
    from pesr_amd.ops import SSIM_WINDOW
    x, y = _shaved(_ssim_luma(out), shave), _shaved(_ssim_luma(lbl), shave)
    mx, my, xx, yy, xy = _ssim_filter(np.stack([x, y, x * x, y * y, x * y]), SSIM_WINDOW)
    c1, c2 = (0.01 * 255) * (0.01 * 255), (0.03 * 255) * (0.03 * 255)
    mxmx, mymy, mxmy = mx * mx, my * my, mx * my
    num = (2.0 * mxmy + c1) * (2.0 * (xy - mxmy) + c2)
    den = ((mxmx + mymy) + c1) * (((xx - mxmx) + (yy - mymy)) + c2)
    return float(np.mean(num / den))


def compute_NIQE(out, model, shave=0):
    """NIQE of an image against a pristine model (a pesr_amd.niqe.NiqeModel or the path of one; docs/modes.md section 4k), a border
    of `shave` pixels dropped first.  No second image is needed.  float32 GPU tensors [N,3,H,W] are measured on the device
    (pesr_amd.niqe.niqe_stats; the mean over the N images comes back); anything else ([1,3,H,W] / [3,H,W] tensors or arrays) goes
    through numpy in float64 with the same definition.  ValueError when the shaved image holds the model's block less than twice or
    fewer than two blocks have finite features."""
    from pesr_amd import niqe as _niqe
    if not isinstance(model, _niqe.NiqeModel):
        model = _niqe.NiqeModel.load(model)
    return float(np.mean(_niqe.niqe(out, model, int(shave))))


def compute_LPIPS(out, lbl, model, shave=0):
    """LPIPS (v0.1, VGG variant; docs/modes.md section 4n) of N image pairs [N,3,H,W] in 0..255 against a pesr_amd.lpips.LpipsModel
    or the path of one, a border of `shave` pixels dropped first -> the mean over the N pairs.  The trunk and the head run on the
    device and there is no CPU path: anything that is not a float32 GPU tensor raises ValueError, as do images that differ in shape
    or are smaller than 16 x 16 after the shave."""
    from pesr_amd import lpips as _lpips
    if not isinstance(model, _lpips.LpipsModel):
        model = _lpips.LpipsModel.load(model)
    return float(_lpips.lpips(out, lbl, model, int(shave)).mean())


def compute_DISTS(out, lbl, model, shave=0):
    """DISTS (docs/modes.md section 4t) of N image pairs [N,3,H,W] in 0..255 against a pesr_amd.dists.DistsModel or the path of one, a
    border of `shave` pixels dropped first -> the mean over the N pairs.  The trunk and the head run on the device and there is no CPU
    path: anything that is not a float32 GPU tensor raises ValueError, as do images that differ in shape or are smaller than 16 x 16
    after the shave."""
    from pesr_amd import dists as _dists
    if not isinstance(model, _dists.DistsModel):
        model = _dists.DistsModel.load(model)
    return float(_dists.dists(out, lbl, model, int(shave)).mean())


def update_tensorboard(epoch, tb, img_idx, inp, out, lbl):
    if tb is None:
        return
    inp, out, lbl = normalize([inp, out, lbl])
    if epoch == 1:
        tb.add_image(f"{img_idx}_LR", inp, epoch)
        tb.add_image(f"{img_idx}_HR", lbl, epoch)
    tb.add_image(f"{img_idx}_SR", out, epoch)


def clean_and_mk_dir(path):
    if os.path.exists(path):
        shutil.rmtree(path)
    os.makedirs(path)
