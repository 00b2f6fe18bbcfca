"""CPU: pesr_amd/quality.py - the Scorer that test.py and train.py's validation share.  Its values are the utils.compute_* calls', its
column order is fixed, its lines are the two programs' own (written out here), and neither its construction nor its refusals touch
the GPU."""
import numpy as np
import pytest
import torch

import lpips_cases as LC
import niqe_cases as NC
import utils
from pesr_amd.niqe import NiqeModel
from pesr_amd.quality import ScoreError, Scorer

TRAIN = dict(flags=("--valid_niqe", "--valid_lpips", "--valid_shave"), size_flags="--valid_shave / --patch_size")


@pytest.fixture
def gpu_untouched(monkeypatch):
    """Every initialisation of torch.cuda from here on is recorded (and refused); the test asserts that there was none."""
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise AssertionError("torch.cuda was initialised")
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    return calls


def _niqe_model():
    return NiqeModel(NC.MODEL_MU, NC.MODEL_COV, 16)


def _pair():
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randint(0, 256, (1, 3, 40, 36), generator=g).float() for _ in range(2))


@pytest.mark.parametrize("shave", [0, 4])
def test_values_are_the_compute_functions_in_column_order(shave):
    sr, hr = _pair()
    model = _niqe_model()
    sc = Scorer("test.py", True, shave, model)
    got = sc.score(sr, hr)
    assert list(got) == sc.columns() == ["PSNR-Y", "SSIM-Y", "NIQE"]
    assert got["PSNR-Y"] == utils.compute_PSNR(sr, hr, shave)
    assert got["SSIM-Y"] == utils.compute_SSIM(sr, hr, shave)
    assert got["NIQE"] == utils.compute_NIQE(sr, model, shave)
    # without an HR image only NIQE comes out; without a model nothing does
    alone = sc.score(sr)
    assert list(alone) == sc.columns(False) == ["NIQE"] and alone["NIQE"] == got["NIQE"]
    assert Scorer("test.py", True, shave).score(sr) == {} and Scorer("test.py", True, shave).columns(False) == []
    # the columns that were not asked for are not there
    plain = Scorer("train.py", False, shave, **TRAIN)
    assert list(plain.score(sr, hr)) == plain.columns() == ["PSNR-Y"]
    # LPIPS is the last column (its value needs the GPU: tests/test_quality_gpu.py)
    assert Scorer("test.py", True, shave, model, LC.model()).columns() == ["PSNR-Y", "SSIM-Y", "NIQE", "LPIPS"]
    assert Scorer("test.py", False, shave, "", LC.model()).columns() == ["PSNR-Y", "LPIPS"]
    # the mean of a set, and of an empty one
    rows = [got, {"PSNR-Y": 1.0, "SSIM-Y": 0.5, "NIQE": 2.0}]
    mean = Scorer.mean(rows)
    assert list(mean) == list(got) and all(mean[c] == float(np.mean([r[c] for r in rows])) for c in got)
    assert Scorer.mean([], sc.columns()) == {"PSNR-Y": 0.0, "SSIM-Y": 0.0, "NIQE": 0.0}


def test_lines_of_both_programs():
    a = {"PSNR-Y": 30.5, "SSIM-Y": 0.9, "NIQE": 5.25, "LPIPS": 0.125}
    b = {"PSNR-Y": 28.25, "SSIM-Y": 0.8, "NIQE": 6.5, "LPIPS": 0.25}
    assert Scorer.test_line(a, b) == ("PSNR-Y 30.5000000000 dB, bicubic 28.2500000000 dB, SSIM-Y 0.9000000000, bicubic 0.8000000000, "
                                      "NIQE 5.2500000000, bicubic 6.5000000000, LPIPS 0.1250000000, bicubic 0.2500000000")
    assert Scorer.test_line({"PSNR-Y": 30.5}, {"PSNR-Y": 28.25}) == "PSNR-Y 30.5000000000 dB, bicubic 28.2500000000 dB"
    assert Scorer.test_line({"NIQE": 5.25}) == "NIQE 5.2500000000"
    assert list(Scorer.valid_lines(3, 20, a, " (EMA)")) == [
        ("Finish valid [3/20]. PSNR: 30.5000dB (EMA)", "Validate PSNR", 30.5),
        ("Finish valid [3/20]. SSIM: 0.900000", "Validate SSIM", 0.9),
        ("Finish valid [3/20]. NIQE: 5.250000", "Validate NIQE", 5.25),
        ("Finish valid [3/20]. LPIPS: 0.125000", "Validate LPIPS", 0.125)]
    assert list(Scorer.valid_lines(1, 1, {"PSNR-Y": 0.0})) == [("Finish valid [1/1]. PSNR: 0.0000dB", "Validate PSNR", 0.0)]


def test_construction_and_refusals_touch_no_gpu(tmp_path, gpu_untouched):
    _niqe_model().save(tmp_path / "m.npz")
    LC.model().save(tmp_path / "w.pt")
    (tmp_path / "junk").write_bytes(b"junk")
    m, w = str(tmp_path / "m.npz"), str(tmp_path / "w.pt")
    with pytest.raises(SystemExit, match=r"test\.py: --niqe .*no such file"):
        Scorer("test.py", False, 0, str(tmp_path / "none.npz"))
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe .*not a NIQE model"):
        Scorer("train.py", False, 0, str(tmp_path / "junk"), **TRAIN)
    with pytest.raises(SystemExit, match=r"test\.py: --lpips .*no such file"):
        Scorer("test.py", False, 0, "", str(tmp_path / "none.pt"))
    with pytest.raises(SystemExit, match=r"train\.py: --valid_lpips .*not readable"):
        Scorer("train.py", False, 0, "", str(tmp_path / "junk"), **TRAIN)
    with pytest.raises(SystemExit, match=r"test\.py: --lpips compares the result with the HR image: it needs --from_hr true"):
        Scorer("test.py", False, 0, m, "x", have_hr=False)
    with pytest.raises(SystemExit, match=r"test\.py: --niqe .*no such file"):         # (the NIQE model is looked at first)
        Scorer("test.py", False, 0, "x", "x", have_hr=False)
    te, tr = Scorer("test.py", True, 4, m, w), Scorer("train.py", True, 2, m, w, **TRAIN)
    assert te.niqe_model.block == 16 and te.lpips_model is not None
    te.check_size(40, 40, "a.png")
    tr.check_size(36, 36, "the synthetic validation images")
    Scorer("test.py", True, 100).check_size(1, 1, "a.png")                              # (PSNR-Y and SSIM-Y refuse when they are measured)
    with pytest.raises(SystemExit, match=r"test\.py: --niqe / --shave: a\.png: .*at least 2"):
        te.check_size(24, 39, "a.png")
    with pytest.raises(SystemExit, match=r"test\.py: --lpips / --shave: a\.png: 12 x 32 after the shave; LPIPS needs at least 16 x 16"):
        Scorer("test.py", False, 4, "", w).check_size(20, 40, "a.png")
    with pytest.raises(SystemExit, match=r"train\.py: --valid_niqe / --valid_shave / --patch_size: the synthetic validation images: .*at least 2"):
        tr.check_size(16, 16, "the synthetic validation images")
    with pytest.raises(SystemExit, match=r"train\.py: --valid_lpips / --valid_shave / --patch_size: the synthetic validation images: 12 x 12 "
                                         r"after the shave; LPIPS needs at least 16 x 16"):
        Scorer("train.py", False, 2, "", w, **TRAIN).check_size(16, 16, "the synthetic validation images")
    with pytest.raises(SystemExit, match=r"0 x 0 after the shave"):
        Scorer("train.py", False, 9, "", w, **TRAIN).check_size(16, 16, "the synthetic validation images")
    # an image that turns out too small when it is scored: the error names the flags for the entry point's own message
    with pytest.raises(ScoreError, match="at least 2") as e:
        tr.score(torch.zeros(1, 3, 20, 20), torch.full((1, 3, 20, 20), 9.0))
    assert e.value.flags == "--valid_niqe / --valid_shave" and isinstance(e.value, ValueError)
    with pytest.raises(ScoreError, match="no CPU path") as e:
        Scorer("test.py", False, 0, "", w).score(torch.zeros(1, 3, 32, 32), torch.full((1, 3, 32, 32), 9.0))
    assert e.value.flags == "--lpips / --shave"
    assert not gpu_untouched
