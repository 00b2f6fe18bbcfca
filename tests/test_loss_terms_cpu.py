"""CPU: the table of optional generator-loss terms (pesr_amd/loss_terms.py, docs/modes.md section 4s) as Trainer and train.py read it.

What each term computes is tested where it was (tests/test_{lpips_loss,ssim_loss,texture,contextual}_{cpu,gpu}.py); here: the table's
shape, the rules that hold for every term, and that a term appended to the table reaches train.py's function and the Trainer with no
other edit.  No test touches the GPU."""
import importlib.util
import os

import pytest
import torch

from pesr_amd import loss_terms
from pesr_amd.loss_terms import TERMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_loss_terms_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


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


def test_the_table(gpu_untouched):
    from pesr_amd import contextual
    from pesr_amd.model.vgg import VGG
    assert [t.key for t in TERMS] == ["lpips", "ssim", "texture", "cx"]            # the order in which the terms join the sum
    assert [t.title for t in TERMS] == ["LPIPS Loss", "SSIM Loss", "Texture Loss", "Contextual Loss"]
    assert len({t.title for t in TERMS}) == len(TERMS)
    assert [t.flag for t in TERMS] == ["--alpha_lpips", "--alpha_ssim", "--alpha_texture", "--alpha_cx"]
    assert [t.phases for t in TERMS] == [("train",), ("pretrain", "train"), ("train",), ("train",)]
    assert [t.taps for t in TERMS] == [(), (), VGG.TAPS, (contextual.TAP,)]
    assert [dict(t.params) for t in TERMS] == [{"lpips_model": None}, {}, {"texture_patch": 16}, {"cx_h": 0.5}]
    assert not gpu_untouched


@pytest.mark.parametrize("term", TERMS, ids=[t.key for t in TERMS])
def test_every_term_is_off_by_default_and_refuses_a_negative_or_nan_weight(term, gpu_untouched):
    from pesr_amd.step import Trainer
    Tr = _load("train")
    parser = Tr.build_parser()
    assert parser.get_default(term.weight) == 0 and term.flag in parser._option_string_actions
    for name, default in term.params.items():                        # a parameter that is a flag has the record's default
        if "--" + name in parser._option_string_actions:
            assert parser.get_default(name) == default, name
    tr = Trainer(None)
    assert tr.terms == [] and getattr(tr, "use_" + term.key) is False and getattr(tr, term.weight) == 0.0
    assert not term().on and not term(**{term.weight: 0.0}).on
    for bad in (-1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=term.weight):
            Trainer(None, **{term.weight: bad})
        with pytest.raises(ValueError, match=term.weight):
            term(**{term.weight: bad})
        for phase in ("pretrain", "train"):
            with pytest.raises(SystemExit, match=rf"^train\.py: {term.flag} {bad} must be >= 0"):
                Tr.loss_terms_of(parser.parse_args([term.flag, str(bad), "--phase", phase]))
    # off: nothing else is checked - a side that no term takes (10), either phase
    for phase in ("pretrain", "train"):
        for extra in ([], ["--scale", "2", "--patch_size", "5"]):
            kw = Tr.loss_terms_of(parser.parse_args(["--patch_size", "10", "--phase", phase] + extra))
            assert kw[term.weight] == 0.0 and Trainer(None, **kw).terms == []
    assert not gpu_untouched


def test_the_keyword_arguments_are_the_records(gpu_untouched):
    from pesr_amd.step import Trainer
    Tr = _load("train")
    kw = Tr.loss_terms_of(Tr.build_parser().parse_args(["--alpha_ssim", "0.5", "--alpha_texture", "2", "--texture_patch", "8", "--alpha_cx", "0.25",
                                                        "--cx_h", "0.1", "--patch_size", "8"]))
    assert kw == {"alpha_lpips": 0.0, "lpips_model": None, "alpha_ssim": 0.5, "alpha_texture": 2.0, "texture_patch": 8, "alpha_cx": 0.25,
                  "cx_h": 0.1}
    tr = Trainer(None, **kw)
    assert [t.key for t in tr.terms] == ["ssim", "texture", "cx"] and [t.alpha for t in tr.terms] == [0.5, 2.0, 0.25]
    assert (tr.use_lpips, tr.use_ssim, tr.use_texture, tr.use_cx) == (False, True, True, True)
    assert (tr.alpha_lpips, tr.alpha_ssim, tr.alpha_texture, tr.alpha_cx) == (0.0, 0.5, 2.0, 0.25)
    assert (tr.lpips_model, tr.texture_patch, tr.cx_h) == (None, 8, 0.1)
    with pytest.raises(TypeError, match="alpha_nothing"):
        Trainer(None, alpha_nothing=1.0)
    assert not gpu_untouched


class _Dummy(loss_terms.Term):
    """A fifth term as a new one would be written: no taps, one parameter, both phases; its value runs on the CPU."""
    key, title = "dummy", "Dummy Loss"
    params = {"dummy_gain": 2.0}
    phases = ("pretrain", "train")

    def check(self, side, what=None):
        return f"--alpha_dummy {self.alpha}: {what or side} is odd" if side % 2 else None

    def value(self, sr, hr, taps_sr, taps_hr):
        assert list(taps_sr) == list(taps_hr) == []
        return self.dummy_gain * (sr.double() - hr.double()).abs().mean(dim=(1, 2, 3))


def test_a_term_appended_to_the_table_reaches_train_py_and_the_trainer(monkeypatch, gpu_untouched):
    """The property the table is for: the record and its flags are all a new term needs."""
    from pesr_amd.step import Trainer
    monkeypatch.setattr(loss_terms, "TERMS", TERMS + (_Dummy,))
    assert _Dummy.flag == "--alpha_dummy" and _Dummy.weight == "alpha_dummy"
    Tr = _load("train")
    parser = Tr.build_parser()
    parser.add_argument("--alpha_dummy", type=float, default=0.0)      # the parser is the one other place a new term touches
    parser.add_argument("--dummy_gain", type=float, default=2.0)
    off = Tr.loss_terms_of(parser.parse_args([]))
    assert off["alpha_dummy"] == 0.0 and Trainer(None, **off).terms == [] and Trainer(None, **off).use_dummy is False
    kw = Tr.loss_terms_of(parser.parse_args(["--alpha_dummy", "0.5", "--dummy_gain", "3", "--alpha_ssim", "1", "--phase", "pretrain"]))
    assert kw["alpha_dummy"] == 0.5 and kw["dummy_gain"] == 3.0
    tr = Trainer(None, **kw)
    assert [t.key for t in tr.terms] == ["ssim", "dummy"] and isinstance(tr.terms[1], _Dummy)      # table order
    assert tr.use_dummy is True and tr.alpha_dummy == 0.5 and tr.dummy_gain == 3.0
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_dummy nan must be >= 0"):
        Tr.loss_terms_of(parser.parse_args(["--alpha_dummy", "nan"]))
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_dummy 1\.0: \(--patch_size \* --scale\) = 5 \* 3 = 15 is odd"):
        Tr.loss_terms_of(parser.parse_args(["--alpha_dummy", "1", "--patch_size", "5", "--scale", "3"]))
    with pytest.raises(ValueError, match="alpha_dummy"):
        Trainer(None, alpha_dummy=-1.0)
    # its loss is weight * the batch mean of its value, as every term's
    sr, hr = torch.full((2, 3, 4, 4), 5.0), torch.full((2, 3, 4, 4), 1.0)
    got = tr.terms[1].loss(sr, hr, [], [])
    assert got.dtype == torch.float32 and got.item() == 0.5 * 3.0 * 4.0
    assert not gpu_untouched
