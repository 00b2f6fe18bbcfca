"""CPU: train.py --resize_jitter and test.py --resize_jitter refuse what they cannot do with a message naming the flags, before any
GPU work (docs/modes.md section 4m)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_resize_jitter_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_train_refuses_resize_jitter_without_its_companions():
    Tm = _load("train")
    full = ["--degradation", "classical", "--lr_from_hr", "true", "--gpu_pipeline", "true", "--resize_jitter", "0.5,2"]
    spec = Tm.degradation_spec(Tm.build_parser().parse_args(full))
    assert (spec.jitter_lo, spec.jitter_hi, spec.jpeg_hi) == (0.5, 2.0, 0) and len(spec) == 4
    assert spec.fields()[-3:] == ("jitter_r", "jitter_m1", "jitter_m2")
    both = Tm.degradation_spec(Tm.build_parser().parse_args(full + ["--jpeg_quality", "30,95", "--noise_sigma", "10"]))
    assert (both.jitter_lo, both.jitter_hi, both.jpeg_lo, both.jpeg_hi, both.noise_hi) == (0.5, 2.0, 30, 95, 10.0)
    assert both.fields()[5:] == ("jpeg_quality", "jitter_r", "jitter_m1", "jitter_m2")
    off = Tm.degradation_spec(Tm.build_parser().parse_args(full[:6]))
    assert (off.jitter_lo, off.jitter_hi) == (0.0, 0.0) and len(off.fields()) == 5
    for argv in (["--resize_jitter", "0.5,2"],                                                               # bicubic
                 ["--resize_jitter", "0.5,2", "--lr_from_hr", "true", "--gpu_pipeline", "true"],
                 ["--resize_jitter", "0.5,2", "--degradation", "classical", "--gpu_pipeline", "true"],
                 ["--resize_jitter", "0.5,2", "--degradation", "classical", "--lr_from_hr", "true"],
                 full + ["--synthetic", "8"]):
        with pytest.raises(SystemExit, match="--resize_jitter .*--degradation classical --lr_from_hr true --gpu_pipeline true"):
            Tm.degradation_spec(Tm.build_parser().parse_args(argv))
    for bad in ("0.5", "0.5,2,3", "a,b", "0.1,2", "0.5,9", "2,0.5", "0,0", "nan,2", "0.5,inf", ","):
        with pytest.raises(SystemExit, match="--resize_jitter"):
            Tm.degradation_spec(Tm.build_parser().parse_args(full[:6] + ["--resize_jitter", bad]))


def test_test_refuses_resize_jitter_it_cannot_apply():
    T = _load("test")
    p = T.build_parser()
    cl = ["--from_hr", "true", "--degradation", "classical"]
    assert T.resize_jitter(p.parse_args([])) is None and T.resize_jitter(p.parse_args(cl)) is None
    assert T.resize_jitter(p.parse_args(cl + ["--resize_jitter", "0.37"])) == (0.37, 0, 0)
    assert T.resize_jitter(p.parse_args(cl + ["--resize_jitter", "1.6,box"])) == (1.6, 2, 0)
    assert T.resize_jitter(p.parse_args(cl + ["--resize_jitter", "8,bilinear,box"])) == (8.0, 1, 2)
    for argv in (["--resize_jitter", "0.5"], ["--from_hr", "true", "--resize_jitter", "0.5"]):
        with pytest.raises(SystemExit, match="--resize_jitter .* needs --from_hr true --degradation classical"):
            T.resize_jitter(p.parse_args(argv))
    for bad in ("x", "", "0.1", "9", "nan", "inf", "0.5,lanczos", "0.5,box,cubic", "0.5,box,box,box", "0.5,"):
        if bad == "":
            continue                                        # (the empty string is "flag not given")
        with pytest.raises(SystemExit, match="--resize_jitter"):
            T.resize_jitter(p.parse_args(cl + ["--resize_jitter", bad]))
    with pytest.raises(SystemExit, match="lanczos.*bicubic, bilinear, box"):
        T.resize_jitter(p.parse_args(cl + ["--resize_jitter", "0.5,lanczos"]))
    # --degradation classical without --from_hr is refused as before, whichever flag is looked at first
    with pytest.raises(SystemExit, match="--from_hr true"):
        T.classical_kernel(p.parse_args(["--degradation", "classical", "--resize_jitter", "0.5"]))
