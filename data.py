"""Minimal data harness so that train.py / test.py run (the reference's data.py - PNG->npy cache, DIV2K/PIRM layout -
is OUT OF SCOPE; benchmarks use synthetic crops).  Two datasets with the reference's sample contract
(reference data.py:79-126): `(lr, hr)` float CHW tensors holding raw 0..255 values, hr = 4x lr, 8-way flip/transpose
augmentation, random LR-aligned crops.  hr = scale x lr with scale 4 by default (the reference's only setting) and 2 or 3 as
an extension (docs/modes.md section 4e).  FolderSRDataset(lr_from_hr=callable) builds its LR images from HR/ alone (section 4f).
"""
import glob
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

SCALE = 4           # the default scale


def augment(lr, hr, idx):
    """idx in 0..7: bit 2 transpose, bit 1 vertical flip, bit 0 horizontal flip (HWC arrays)."""
    if idx & 4:
        lr, hr = lr.transpose(1, 0, 2), hr.transpose(1, 0, 2)
    if idx & 2:
        lr, hr = lr[::-1], hr[::-1]
    if idx & 1:
        lr, hr = lr[:, ::-1], hr[:, ::-1]
    return np.ascontiguousarray(lr), np.ascontiguousarray(hr)


def to_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32))


class SyntheticSRDataset(Dataset):
    """DIV2K-shaped random crops: iid integers 0..255.  Deterministic per index."""

    def __init__(self, length, patch_size, seed=1234, scale=SCALE):
        self.length, self.ps, self.seed, self.scale = length, patch_size, seed, scale

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + i)
        lr = torch.randint(0, 256, (3, self.ps, self.ps), generator=g).float()
        hr = torch.randint(0, 256, (3, self.scale * self.ps, self.scale * self.ps), generator=g).float()
        return lr, hr


class FolderSRDataset(Dataset):
    """<root>/LR/*.png with matching <root>/HR/*.png (PIL); random crop + augmentation when patch_size is given.  Every HR image
    must be exactly scale x its LR image (ValueError naming the file otherwise).
    With a callable `lr_from_hr(hr uint8 HWC array) -> lr uint8 HWC array`, LR/ is not consulted: the file list comes from
    HR/*.png, every HR image is cropped at the top-left to multiples of `scale` and its LR image is made ONCE, here, and kept in
    host memory (HR is still read per item).  The dataset holds no GPU code: the caller supplies the resize (train.py: the device
    bicubic of docs/modes.md section 4f, called in the parent process before the loader's workers fork).  With `lr_from_hr_index`
    the callable is `lr_from_hr(hr, i)`, i the image's position in the sorted file list (the classical degradation of section 4j
    gives every validation image parameters of its own that way)."""

    def __init__(self, root, patch_size=None, num_repeats=1, is_aug=False, fixed_length=None, scale=SCALE, lr_from_hr=None,
                 lr_from_hr_index=False):
        from PIL import Image
        self._open = Image.open
        self.ps, self.rep, self.aug, self.scale = patch_size, num_repeats, is_aug, scale
        self.lr_images = None
        if lr_from_hr is not None:
            self.hr_paths = sorted(glob.glob(os.path.join(root, "HR", "*.png")))
            if fixed_length:
                self.hr_paths = self.hr_paths[:fixed_length]
            self.lr_paths = self.hr_paths                     # (one entry per sample; never opened)
            self.lr_images = [np.ascontiguousarray(lr_from_hr(self._read_hr(p), i) if lr_from_hr_index else lr_from_hr(self._read_hr(p)))
                              for i, p in enumerate(self.hr_paths)]
            return
        self.lr_paths = sorted(glob.glob(os.path.join(root, "LR", "*.png")))
        if fixed_length:
            self.lr_paths = self.lr_paths[:fixed_length]
        self.hr_paths = [os.path.join(root, "HR", os.path.basename(p)) for p in self.lr_paths]

    def _read_hr(self, path):
        hr = np.asarray(self._open(path).convert("RGB"))
        s = self.scale
        return np.ascontiguousarray(hr[:hr.shape[0] - hr.shape[0] % s, :hr.shape[1] - hr.shape[1] % s])

    def __len__(self):
        return len(self.lr_paths) * self.rep

    def __getitem__(self, i):
        i %= len(self.lr_paths)
        if self.lr_images is not None:
            lr, hr = self.lr_images[i], self._read_hr(self.hr_paths[i])
        else:
            lr = np.asarray(self._open(self.lr_paths[i]).convert("RGB"))
            hr = np.asarray(self._open(self.hr_paths[i]).convert("RGB"))
        s = self.scale
        if hr.shape[:2] != (s * lr.shape[0], s * lr.shape[1]):
            raise ValueError(f"{self.hr_paths[i]}: HR image is {hr.shape[1]}x{hr.shape[0]}, expected {s} x the LR image "
                             f"{lr.shape[1]}x{lr.shape[0]} = {s * lr.shape[1]}x{s * lr.shape[0]} (scale {s})")
        if self.ps:
            y = random.randint(0, lr.shape[0] - self.ps)
            x = random.randint(0, lr.shape[1] - self.ps)
            lr = lr[y:y + self.ps, x:x + self.ps]
            hr = hr[s * y:s * (y + self.ps), s * x:s * (x + self.ps)]
        if self.aug:
            lr, hr = augment(lr, hr, random.randint(0, 7))
        return to_tensor(lr), to_tensor(hr)
