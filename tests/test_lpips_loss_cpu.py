"""CPU: LPIPS as a training loss (docs/modes.md section 4o) - the head's gradient restated (tests/lpips_grad_oracle.py) against
torch.autograd on the float64 definition, the kernel's order against the formula within the derived bound, the rule at all-zero
pixels, and the refusals of train.py's flags and of lpips_loss's shapes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lpips_cases as C
import lpips_grad_cases as G
import lpips_grad_oracle as GO
import lpips_oracle as LO
from pesr_amd import lpips as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_lpips_loss_" + name, os.path.join(ROOT, name + ".py"))
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


def _autograd(fa, fb, w, g):
    """d(sum_n g[n] score[n]) / d fa by torch.autograd on the float64 definition, the arithmetic of lpips_oracle._metric's head."""
    a = torch.from_numpy(np.array(fa)).double().requires_grad_()
    b = torch.from_numpy(np.array(fb)).double()
    wt = torch.from_numpy(np.array(w)).double()
    ah = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + LO.EPS)
    bh = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + LO.EPS)
    score = (wt * (ah - bh).pow(2)).sum(-1).mean(dim=(1, 2))
    (score * torch.from_numpy(np.array(g))).sum().backward()
    return a.grad.numpy()


def _worst(diff, allow):
    """The largest diff / allow over the elements with a positive allowance; elements whose allowance is 0 must not differ at all."""
    assert bool((diff[allow == 0] == 0).all())
    pos = allow > 0
    return float(np.max(diff[pos] / allow[pos])) if pos.any() else 0.0


# ---- 1. the formula is the derivative of the definition -----------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,h,w", G.SPECIAL)
def test_grad_exact_is_autograd_of_the_float64_definition(c, n, h, w):
    for kind in ("relu", "near", "wzeros", "zeros"):
        fa, fb, wt, g = G.case(c, n, h, w, kind)
        exact, bound = G.exact_and_bound(c, n, h, w, kind)
        auto = _autograd(fa, fb, wt, g)
        live = np.sqrt((fa.astype(np.float64) ** 2).sum(-1)) > 0         # the pixels with na > 0
        assert live.any() or kind == "zeros"
        ratio = _worst(np.abs(auto - exact)[live], bound[live])
        print(f"C {c} {n} x {h} x {w} {kind}: max |autograd - grad_exact| / grad_bound = {ratio:.3f} over {int(live.sum())} pixels, "
              f"max |grad| {np.abs(exact).max():.3e}")
        assert np.isfinite(auto[live]).all() and ratio <= 1.0
        if kind == "zeros":
            # THE RULE AT na == 0 IS A CHOICE: the restatement gives 0 there, autograd gives something that is not a number
            dead = ~live
            assert dead.any()
            assert bool((exact[dead] == 0).all()) and bool((GO.grad_ordered(fa, fb, wt, g)[dead] == 0).all())
            assert not np.isfinite(auto[dead]).any()


def test_rule_at_an_all_zero_pixel_is_a_choice():
    """One pixel built by hand: a all zero, b not.  grad_exact and grad_ordered are 0 there; autograd is non-finite; the formula's own
    value would be 2 g w_j t_j / (H W 1e-10)."""
    fa, fb, wt, g = (np.array(t) for t in G.case(64, 1, 4, 4, "relu"))
    fa[0, 2, 1, :] = 0.0
    assert fb[0, 2, 1].max() > 0
    exact, ordered, auto = GO.grad_exact(fa, fb, wt, g), GO.grad_ordered(fa, fb, wt, g), _autograd(fa, fb, wt, g)
    assert bool((exact[0, 2, 1] == 0).all()) and bool((ordered[0, 2, 1] == 0).all())
    assert not np.isfinite(auto[0, 2, 1]).any()
    others = np.ones((4, 4), bool)
    others[2, 1] = False
    assert np.isfinite(auto[0][others]).all() and np.abs(exact[0][others]).max() > 0


# ---- 2. the kernel's order against the formula ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,h,w", G.SPECIAL)
def test_grad_ordered_within_the_derived_bound_of_grad_exact(c, n, h, w):
    for kind in G.KINDS:
        fa, fb, wt, g = G.case(c, n, h, w, kind)
        exact, bound = G.exact_and_bound(c, n, h, w, kind)
        got = G.ordered(c, n, h, w, kind)
        assert got.dtype == np.float32 and got.shape == exact.shape and np.isfinite(got).all()
        allow = GO.fp32_allowance(exact, bound)
        allow[bound == 0] = np.where(exact[bound == 0] == 0, 0.0, allow[bound == 0])
        ratio = _worst(np.abs(got.astype(np.float64) - exact), allow)
        print(f"C {c} {n} x {h} x {w} {kind}: max |grad_ordered - grad_exact| / (grad_bound + one fp32 rounding) = {ratio:.3f}, "
              f"max bound / |exact| {float(np.max(bound[exact != 0] / np.abs(exact[exact != 0]))) if (exact != 0).any() else 0.0:.3e}")
        assert ratio <= 1.0
        if kind == "same":
            assert bool((got == 0).all()) and bool((exact == 0).all())
        if kind == "near":
            # t cancels: |t| is 1e-4 of |ah|, and the bound, absolute in t, is still far below the gradient itself
            assert float(np.median(bound[exact != 0] / np.abs(exact[exact != 0]))) < 1e-9
        if kind == "wzeros":
            assert bool((np.array(wt) == 0).any()) and np.abs(got[..., np.array(wt) == 0]).max() > 0      # -(a_j / na) q / da remains


def test_distinct_g_per_image_and_linearity():
    fa, fb, wt, g = G.case(128, 2, 3, 5, "relu")
    assert g[0] != g[1]
    base = GO.grad_ordered(fa, fb, wt, g)
    for n in range(2):
        one = GO.grad_ordered(fa[n:n + 1], fb[n:n + 1], wt, g[n:n + 1])
        assert np.array_equal(one[0], base[n])                       # images do not mix
    zero = GO.grad_ordered(fa, fb, wt, np.array([0.0, g[1]]))
    assert bool((zero[0] == 0).all()) and np.array_equal(zero[1], base[1])


def test_trunk_gradient_seeds_meet_their_conditions():
    """The image seeds of the device's end-to-end gradient test are chosen HERE, on the CPU, by conditions on the float64 run and on the
    CPU's own float32 run (tests/lpips_trunk_grad.py): never by what the device gives."""
    import lpips_trunk_grad as T
    for shape, seed in T.TRUNK_CASES:
        r = T.reference(shape, seed)
        print(f"{shape} seed {seed}: ties {r['ties']}, kink mass {r['kink_mass']:.4f}, closest gradient-carrying pre-activation "
              f"{r['closest']:.2e}, float32 trunk error {r['e_ref']:.3e} of the maximum {r['gmax']:.3e}")
        assert r["ties"] == 0 and r["kink_mass"] <= T.KINK_MASS and T.holds(r)
        assert r["gmax"] > 0 and np.isfinite(r["g64"]).all() and r["g64"].shape == shape
    bad = T.reference((2, 3, 32, 48), 0)                             # a seed that is refused: a gradient-carrying pre-activation at 1.8e-8
    assert not T.holds(bad) and bad["closest"] < T.KINK_CLOSEST


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_lpips_loss_refuses_sides_that_are_no_multiple_of_16(gpu_untouched):
    m = C.model()
    for shape, shave in (((1, 3, 24, 20), 0), ((1, 3, 32, 24), 0), ((2, 3, 40, 40), 3), ((1, 3, 16, 8), 0), ((1, 3, 32, 32), 7)):
        x = torch.zeros(shape)
        with pytest.raises(ValueError, match=r"multiples of 16 .*max-pool backward takes even sides only"):
            LP.lpips_loss(x, x, m, shave)
    with pytest.raises(ValueError, match=r"24 x 20"):
        LP.lpips_loss(torch.zeros(1, 3, 24, 20), torch.zeros(1, 3, 24, 20), m)
    with pytest.raises(ValueError, match="differ in shape"):
        LP.lpips_loss(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 16), m)
    with pytest.raises(ValueError, match="no CPU path"):
        LP.lpips_loss(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), m)          # a shape it takes, on the CPU
    with pytest.raises(ValueError, match="no CPU path"):
        LP.lpips_loss(torch.zeros(1, 3, 32, 32).double(), torch.zeros(1, 3, 32, 32).double(), m)
    assert LP.check_loss_side(192, 192) is None and LP.check_loss_side(16, 48) is None and LP.check_loss_side(0, 16) is not None
    assert not gpu_untouched


def test_c_abi_of_the_gradient_refuses_before_anything_is_launched():
    """pesr_lpips_layer_bwd and pesr_lpips_layer2 check their arguments on the host first (the pointers are never followed there)."""
    from pesr_amd import _lib
    lib = _lib.lib()
    assert "pesr_lpips_layer_bwd" in _lib.SIGNATURES and "pesr_lpips_layer2" in _lib.SIGNATURES
    p, big = 0x10000, 1 << 40
    bwd = lambda N, H, W, Cc, fa=p, fb=p, w=p, g=p, ga=p: lib.pesr_lpips_layer_bwd(fa, fb, w, g, ga, N, H, W, Cc, None)
    fwd = lambda N, H, W, Cc, fa=p, fb=p, ws=p, nb=big: lib.pesr_lpips_layer2(fa, fb, p, p, N, H, W, Cc, None, ws, nb, None)
    for call in (bwd, fwd):
        for c in (96, 0, 32, 63, 192, 1024, -64):
            assert call(1, 8, 8, c) == -1, c
        assert call(0, 8, 8, 64) == -1 and call(65536, 8, 8, 64) == -1 and call(1, 0, 8, 64) == -1 and call(1, 8, 0, 64) == -1
        assert call(1, 8, 8, 64, fa=None) == -1 and call(1, 8, 8, 64, fb=None) == -1
        assert call(1, 8, 8, 64, fa=p + 4) == -1 and call(1, 8, 8, 64, fb=p + 8) == -1
    assert bwd(1, 8, 8, 64, ga=p + 8) == -1 and bwd(1, 8, 8, 64, ga=None) == -1 and bwd(1, 8, 8, 64, g=p + 4) == -1
    assert bwd(1, 8, 8, 64, g=None) == -1 and bwd(1, 8, 8, 64, w=p + 2) == -1
    assert fwd(2, 9, 7, 64, nb=8 * 2 * 1 - 1) == -2 and fwd(1, 8, 8, 64, ws=None, nb=0) == -2
    assert lib.pesr_abi_version() == 20


def test_train_flags_default_off_and_refusals(tmp_path, monkeypatch, gpu_untouched):
    Tr = _load("train")
    d = Tr.build_parser().parse_args([])
    assert d.lpips_loss == "" and d.alpha_lpips == 0.0
    assert Tr.loss_terms_of(d)["lpips_model"] is None
    C.model().save(tmp_path / "w.pt")
    (tmp_path / "junk.pt").write_bytes(b"junk")
    monkeypatch.chdir(tmp_path)
    w = str(tmp_path / "w.pt")
    with pytest.raises(SystemExit, match=r"train\.py: --alpha_lpips 0\.5 needs --lpips_loss"):
        Tr.main(["--alpha_lpips", "0.5", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"train\.py: --lpips_loss .*no such file"):
        Tr.main(["--alpha_lpips", "0.5", "--lpips_loss", str(tmp_path / "none.pt"), "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"train\.py: --lpips_loss .*not readable"):
        Tr.main(["--lpips_loss", str(tmp_path / "junk.pt"), "--synthetic", "16"])       # the file must load even with the term off
    with pytest.raises(SystemExit, match=r"train\.py: --alpha_lpips 0\.5 / --lpips_loss: .*--phase train, not --phase pretrain"):
        Tr.main(["--alpha_lpips", "0.5", "--lpips_loss", w, "--phase", "pretrain", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"train\.py: --alpha_lpips / --lpips_loss: \(--patch_size \* --scale\) = 10 \* 4 = 40: .*multiples of 16"):
        Tr.main(["--alpha_lpips", "0.5", "--lpips_loss", w, "--patch_size", "10", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"train\.py: --alpha_lpips / --lpips_loss: .*= 12 \* 2 = 24: .*multiples of 16"):
        Tr.main(["--alpha_lpips", "0.5", "--lpips_loss", w, "--patch_size", "12", "--scale", "2", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"train\.py: --alpha_lpips -1\.0 must be >= 0"):
        Tr.main(["--alpha_lpips", "-1", "--lpips_loss", w, "--synthetic", "16"])
    # what passes, and the sharing with --valid_lpips
    ok = Tr.build_parser().parse_args(["--alpha_lpips", "0.5", "--lpips_loss", w, "--patch_size", "12", "--valid_lpips", w])
    valid = Tr.lpips_model_of(ok)
    assert Tr.loss_terms_of(ok, valid)["lpips_model"] is valid
    other = Tr.loss_terms_of(ok, None)["lpips_model"]
    assert isinstance(other, LP.LpipsModel) and other is not valid
    off = Tr.build_parser().parse_args(["--lpips_loss", w])
    assert Tr.loss_terms_of(off)["lpips_model"] is None                       # a weight file alone turns nothing on
    assert not gpu_untouched


def test_trainer_term_is_off_without_both_arguments():
    from pesr_amd.step import Trainer
    m = C.model()
    assert not Trainer(None).use_lpips and not Trainer(None, lpips_model=m).use_lpips and not Trainer(None, alpha_lpips=1.0).use_lpips
    assert Trainer(None, lpips_model=m, alpha_lpips=0.25).use_lpips
    with pytest.raises(ValueError, match="alpha_lpips"):
        Trainer(None, lpips_model=m, alpha_lpips=-1.0)
