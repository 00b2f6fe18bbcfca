"""GPU: pesr_amd/quality.py on the device - the Scorer's four values are the utils.compute_* calls' own, and the two facts that let
test.py and train.py share it: PSNR-Y and SSIM-Y do not depend on the order of their two images, bit for bit, and LPIPS of an
integer-valued image is LPIPS of its clamped and rounded copy."""
import numpy as np
import pytest
import torch

import lpips_cases as LC
import niqe_cases as NC
import utils
from pesr_amd import ops
from pesr_amd.niqe import NiqeModel
from pesr_amd.quality import Scorer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPE = (1, 3, 48, 40)      # shave 4 leaves 40 x 32: above LPIPS's 16, SSIM's 11-pixel window and two 16-pixel NIQE blocks


def _pair():
    """(a Generator's result: non-integer values, some outside 0..255; the HR image; the integer-valued copy of the result)."""
    a, b = LC.image_pair(SHAPE)
    off = np.random.default_rng(3).uniform(-0.5, 0.5, a.shape) + np.where(a > 250, 9.0, 0.0) - np.where(a < 5, 9.0, 0.0)
    return tuple(torch.from_numpy(np.array(t, dtype=np.float32)).to(DEV) for t in (a + off, b, a))


@pytest.mark.parametrize("shave", [0, 4])
def test_scorer_values_are_the_compute_functions(shave):
    sr, hr, _ = _pair()
    niqe, lpips = NiqeModel(NC.MODEL_MU, NC.MODEL_COV, 16), LC.model()
    got = Scorer("test.py", True, shave, niqe, lpips).score(sr, hr)
    assert list(got) == ["PSNR-Y", "SSIM-Y", "NIQE", "LPIPS"]
    assert got["PSNR-Y"] == utils.compute_PSNR(sr, hr, shave)
    assert got["SSIM-Y"] == utils.compute_SSIM(sr, hr, shave)
    assert got["NIQE"] == utils.compute_NIQE(sr, niqe, shave)
    assert got["LPIPS"] == utils.compute_LPIPS(sr.clamp(0, 255).round(), hr, lpips, shave)
    assert all(np.isfinite(v) for v in got.values()) and got["LPIPS"] > 0
    assert Scorer("train.py", False, shave, niqe).score(sr) == {"NIQE": got["NIQE"]}


@pytest.mark.parametrize("shave", [0, 4])
def test_psnr_and_ssim_do_not_depend_on_the_operand_order(shave):
    sr, hr, _ = _pair()
    a = sr[..., shave:SHAPE[2] - shave, shave:SHAPE[3] - shave]
    b = hr[..., shave:SHAPE[2] - shave, shave:SHAPE[3] - shave]
    assert torch.equal(ops.psnr_y(a, b), ops.psnr_y(b, a))
    assert torch.equal(ops.ssim_y(sr, hr, shave), ops.ssim_y(hr, sr, shave))
    # and in both memory formats, as train.py's validation hands them over (the result channels_last, the HR image not)
    cl = sr.contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.ssim_y(cl, hr, shave), ops.ssim_y(hr, cl, shave))
    assert utils.compute_PSNR(cl, hr, shave) == utils.compute_PSNR(hr, cl, shave)
    assert utils.compute_SSIM(cl, hr, shave) == utils.compute_SSIM(hr, cl, shave)


def test_lpips_of_an_integer_image_is_that_of_its_rounded_copy():
    _, hr, sr = _pair()
    assert torch.equal(sr, sr.clamp(0, 255).round())
    for shave in (0, 4):
        assert utils.compute_LPIPS(sr, hr, LC.model(), shave) == utils.compute_LPIPS(sr.clamp(0, 255).round(), hr, LC.model(), shave)
