"""GPU: what holds for every optional term of the generator's loss (pesr_amd/loss_terms.py TERMS, docs/modes.md section 4s), asserted once
for all of them: off, the step is the step without the term's arguments; on, the first step's other logs keep their bits, G moves and D's
first step is untouched; two eager steps, a capture and two replays give the bits of four eager steps.  Then all terms at once.

What a term's value IS stays with its own file (tests/test_{lpips_loss,ssim_loss,texture,contextual}_gpu.py), which runs on the same
harness (tests/loss_step_harness.py) with the same numbers, so the runs here are the runs there.  Shapes: the toy networks of those
files - 64 channels, 2 blocks, LR 8 x 8, HR 32 x 32 (a multiple of 16 for LPIPS, at least 11 for SSIM, texture patches of 8 divide 32, 16
and 8, a contextual tap of 8 x 8 = 64 points)."""
import pytest

import loss_step_harness as HS
from pesr_amd.loss_terms import TERMS

pytestmark = pytest.mark.gpu
MODEL = "the shared LpipsModel.random"                               # (made when a test first needs it, not at collection)

# key -> the harness (seed, batch) of the term's own file, argument sets with the term off, argument sets with it on
CASES = {
    "lpips": ((150, 4), {"alpha0": {"alpha_lpips": 0.0}, "alpha0+model": {"lpips_model": MODEL, "alpha_lpips": 0.0}, "no-model": {"alpha_lpips": 1.0}},
              {"on": {"lpips_model": MODEL, "alpha_lpips": 1.0}}),
    "ssim": ((250, 4), {"alpha0": {"alpha_ssim": 0.0}}, {"on": {"alpha_ssim": 0.5}}),
    "texture": ((350, 2), {"alpha0": {"alpha_texture": 0.0, "texture_patch": 8}},
                {"patch8": {"alpha_texture": 0.5, "texture_patch": 8}, "patch0": {"alpha_texture": 0.5, "texture_patch": 0}}),
    "cx": ((350, 2), {"alpha0": {"alpha_cx": 0.0, "cx_h": 0.25}}, {"on": {"alpha_cx": 0.5}}),
}


def _params(which):
    out = []
    for t in TERMS:
        if t.key in CASES:
            for phase in t.phases:
                out += [pytest.param(t, phase, kw, id=f"{t.key}-{phase}-{name}") for name, kw in CASES[t.key][which].items()]
    return out


def _kw(kw):
    return {k: HS.lpips_model() if v is MODEL else v for k, v in kw.items()}


def _harness(term):
    return HS.harness(*CASES[term.key][0])


def _calls(taps, steps, phase="train"):
    """How the VGG is called in `steps` steps of a trainer whose terms read `taps`."""
    return [] if phase != "train" else [{"taps": taps} if taps else {}] * steps


def test_every_term_of_the_table_has_cases():
    assert sorted(CASES) == sorted(t.key for t in TERMS)
    for t in TERMS:
        assert CASES[t.key][1] and CASES[t.key][2], t.key


@pytest.mark.parametrize("term,phase,kw", _params(1))
def test_step_with_the_term_off_is_the_step_without_it(term, phase, kw):
    HS.assert_off_is_the_step_without(_harness(term), phase, term.key, **_kw(kw))


@pytest.mark.parametrize("term,phase,kw", _params(2))
def test_step_with_the_term_on_leaves_the_rest_alone(term, phase, kw):
    H = _harness(term)
    logs4, states4, calls = H.run(4, phase, **_kw(kw))
    logs0, states0, _ = H.run(2, phase)
    assert calls == _calls(term.taps, 4, phase)
    assert all(term.key in l and l[term.key] > 0 for l in logs4)
    HS.assert_only_G_moved(logs4[0], states4[0], logs0[0], states0[0])


@pytest.mark.parametrize("term,phase,kw", _params(2))
def test_step_with_the_term_on_survives_the_capture(term, phase, kw):
    HS.assert_survives_the_capture(_harness(term), phase, [term.key], **_kw(kw))


# ---- all terms at once -------------------------------------------------------------------------------------------------------------------
ALL = (350, 2)                                                        # the harness of the two terms that read taps: their runs are shared


def _alone(term):
    return next(iter(CASES[term.key][2].values()))


def _all_kw():
    kw = {}
    for t in TERMS:
        kw.update(_kw(_alone(t)))
    return kw


def test_all_terms_at_once_log_what_each_logs_alone():
    H = HS.harness(*ALL)
    logs4, states4, calls = H.run(4, **_all_kw())
    logs0, states0, _ = H.run(2)
    assert calls == [{"taps": (1, 6, 11, 17)}] * 4                    # ONE call per step, tapped at the union
    assert list(logs4[0])[-len(TERMS):] == [t.key for t in TERMS]     # logged in table order, behind the step's own
    for t in TERMS:
        alone, _, _ = H.run(4, **_kw(_alone(t)))
        assert logs4[0][t.key] == alone[0][t.key], t.key              # bit for bit the value of the run with that term alone
    HS.assert_only_G_moved(logs4[0], states4[0], logs0[0], states0[0])


def test_all_terms_at_once_survive_the_capture():
    HS.assert_survives_the_capture(HS.harness(*ALL), "train", [t.key for t in TERMS], **_all_kw())
