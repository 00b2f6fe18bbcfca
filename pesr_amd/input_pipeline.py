"""GPU-side input pipeline: the uint8 image pool lives in HBM; a batch of (LR, HR) training crops with
the reference's 8-way augmentation (reference data.py:79-126) is assembled by one kernel launch per resolution.
Replaces the reference's 4 DataLoader worker processes + pinned-memory copies (reference train.py:96-97) - at
8 x 127 patches/s the host path would have to deliver ~1000 crops/s."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

SCALE = 4           # the default scale (2 and 3 are extensions, docs/modes.md section 4e)


class GpuPatchSampler:
    def __init__(self, lr_images: Sequence[np.ndarray], hr_images: Sequence[np.ndarray], device: torch.device, scale: int = SCALE):
        assert len(lr_images) == len(hr_images) and len(lr_images) > 0
        assert scale in (2, 3, 4), scale
        self.device, self.scale = device, scale
        self.n = len(lr_images)
        self.lr_shapes = [im.shape for im in lr_images]
        for l, h in zip(lr_images, hr_images):
            assert l.dtype == np.uint8 and h.dtype == np.uint8 and l.shape[2] == 3
            assert h.shape[0] == scale * l.shape[0] and h.shape[1] == scale * l.shape[1], f"HR must be {scale}x the LR image"
        self.lr_pool, self.lr_off = self._pool(lr_images)
        self.hr_pool, self.hr_off = self._pool(hr_images)

    @classmethod
    def from_hr(cls, hr_images: Sequence[np.ndarray], device: torch.device, scale: int = SCALE, degradation=None):
        """A sampler from HR images alone: each is mod-cropped to multiples of `scale`, the HR pool is uploaded once and the LR pool
        is made from it on the device (pesr_amd.resize: MATLAB's bicubic imresize, docs/modes.md section 4f) in two launches.
        From there on it is the sampler the constructor would build from (LR, HR).
        With `degradation` (a pesr_amd.degrade.DegradationSpec) there is no LR pool: every pick carries a blur kernel and a noise
        level of its own, and assemble() makes its LR patch from the HR pool on the spot (docs/modes.md section 4j)."""
        from .resize import imresize_pool_u8, modcrop
        assert len(hr_images) > 0 and scale in (2, 3, 4), scale
        self = cls.__new__(cls)
        self.device, self.scale, self.n = device, scale, len(hr_images)
        hrs = [modcrop(im, scale) for im in hr_images]
        for h in hrs:
            assert h.dtype == np.uint8 and h.ndim == 3 and h.shape[2] == 3 and h.shape[0] >= scale and h.shape[1] >= scale
        self.hr_pool, self.hr_off = self._pool(hrs)
        if degradation is not None:
            from .degrade import kernel_size
            self.degradation = degradation
            self.kernel_size = kernel_size(scale, degradation.sigma_hi)
            self.hr_shapes = [h.shape[:2] for h in hrs]
            self.lr_pool = self.lr_off = None
            self.lr_shapes = [(h.shape[0] // scale, h.shape[1] // scale, 3) for h in hrs]
            return self
        self.lr_pool, self.lr_off, lr_hw = imresize_pool_u8(self.hr_pool, self.hr_off, [h.shape[:2] for h in hrs], scale, up=False)
        self.lr_shapes = [(h, w, 3) for h, w in lr_hw]
        return self

    def _pool(self, images):
        offs, total = [], 0
        for im in images:
            offs.append(total)
            total += im.size
        flat = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])
        return torch.from_numpy(flat).to(self.device), offs

    degradation = None      # from_hr(degradation=spec) sets it

    def _pick(self, i, patch, rng, augment):
        h, w, _ = self.lr_shapes[i]
        pick = (i, rng.randint(0, h - patch), rng.randint(0, w - patch), rng.randint(0, 7) if augment else 0)
        # the spec's draw (DegradationSpec.fields() names its values), after the crop and from the same stream
        return pick if self.degradation is None else pick + self.degradation.draw(rng)

    def draw(self, batch: int, patch: int, rng: Optional[random.Random] = None, augment: bool = True):
        """Host-side random choices, as the reference's random.randint calls: (image, y, x, aug) per sample; with a degradation
        spec (image, y, x, aug, sigma1, sigma2, theta, sigma_n, q), then the JPEG quality when the spec has one, then the resize
        jitter's (r, m1, m2) when it has one: DegradationSpec.named(pick[4:]) names them."""
        rng = rng or random
        return [self._pick(rng.randrange(self.n), patch, rng, augment) for _ in range(batch)]

    def draw_for(self, images: Sequence[int], patch: int, rng: Optional[random.Random] = None, augment: bool = True):
        """As draw(), for a GIVEN list of image indices (an epoch permutation dealt out by the caller): only the crop origin
        and the augmentation are random."""
        rng = rng or random
        return [self._pick(i, patch, rng, augment) for i in images]

    def _degraded_patches(self, picks, patch):
        """The step's LR patches, unaugmented, as a scratch uint8 pool of B patches of patch x patch pixels (patch b at byte
        3 * patch * patch * b): every pick's window of the HR pool through degrade.degrade_chain_pool_u8 with the pick's own kernel,
        noise, resize jitter (section 4m: reflection at the patch's own border) and JPEG quality (section 4l: the block grid starts
        at the patch's own origin)."""
        from .degrade import degrade_chain_pool_u8, gaussian_kernel
        spec, B = self.degradation, len(picks)
        drawn = [spec.named(p[4:]) for p in picks]
        bank = np.stack([gaussian_kernel(self.kernel_size, d["sigma1"], d["sigma2"], d["theta"]) for d in drawn])
        column = lambda name: [d[name] for d in drawn]  # noqa: E731
        out, _, _ = degrade_chain_pool_u8(self.hr_pool, [self.hr_off[p[0]] for p in picks], [self.hr_shapes[p[0]] for p in picks], self.scale,
                                          bank, range(B), column("sigma_n"), column("q"), windows=[(p[1], p[2], patch, patch) for p in picks],
                                          jitter=[column(k) for k in ("jitter_r", "jitter_m1", "jitter_m2")] if spec.jitter_hi else None,
                                          jpeg=column("jpeg_quality") if spec.jpeg_hi else None, jpeg_420=spec.jpeg_420)
        return out

    def assemble(self, picks: List[tuple], patch: int, nhwc: bool = False):
        """-> (lr [B,3,P,P], hr [B,3,sP,sP]) fp32 on the device, s = self.scale (logical NCHW; channels_last memory when nhwc)."""
        B, S = len(picks), self.scale
        dl = np.empty((B, 3), dtype=np.int64)
        dh = np.empty((B, 3), dtype=np.int64)
        lr_pool = self.lr_pool
        if self.degradation is not None:
            lr_pool = self._degraded_patches(picks, patch)
        for b, (i, y, x, aug) in enumerate(p[:4] for p in picks):
            w = self.lr_shapes[i][1]
            if self.degradation is not None:            # patch b of the scratch pool, whole: origin (0, 0), stride `patch`
                dl[b] = (3 * patch * patch * b, patch, aug << 32)
            else:
                dl[b] = (self.lr_off[i], w | (y << 32), x | (aug << 32))
            dh[b] = (self.hr_off[i], (S * w) | ((S * y) << 32), (S * x) | (aug << 32))
        L = _lib.lib()
        s = torch.cuda.current_stream(self.device).cuda_stream
        outs = []
        for pool, d, P in ((lr_pool, dl, patch), (self.hr_pool, dh, S * patch)):
            desc = torch.from_numpy(d).to(self.device)
            out = torch.empty((B, P, P, 3) if nhwc else (B, 3, P, P), dtype=torch.float32, device=self.device)
            _lib.check(L.pesr_crop_augment(pool.data_ptr(), desc.data_ptr(), out.data_ptr(), B, P, int(nhwc), s), "pesr_crop_augment")
            outs.append(out.permute(0, 3, 1, 2) if nhwc else out)
        return outs[0], outs[1]

    def sample(self, batch: int, patch: int, rng: Optional[random.Random] = None, augment: bool = True, nhwc: bool = False):
        return self.assemble(self.draw(batch, patch, rng, augment), patch, nhwc)
