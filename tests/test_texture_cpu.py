"""CPU: the texture loss (docs/modes.md section 4q) - the restatement's gradient formula (tests/texture_oracle.py) against
torch.autograd on the float64 definition, the refusals of the C entry points, of the ops, of train.py --alpha_texture and of the
Trainer, and the patch rule."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import texture_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_texture_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _definition(fa, fb, ph, pw):
    """The definition with torch ops in float64, independent of the oracle's einsum: [N] per image"""
    n, h, w, c = fa.shape
    out = []
    for i in range(n):
        t = fa.new_zeros(())
        for py in range(h // ph):
            for px in range(w // pw):
                a = fa[i, py * ph:(py + 1) * ph, px * pw:(px + 1) * pw].reshape(-1, c)
                b = fb[i, py * ph:(py + 1) * ph, px * pw:(px + 1) * pw].reshape(-1, c)
                d = (a.t() @ a - b.t() @ b) / (c * ph * pw)
                t = t + (d * d).sum()
        out.append(t / ((h // ph) * (w // pw)))
    return torch.stack(out)


# ---- 1. the gradient formula is the derivative of the definition ----------------------------------------------------------------------
@pytest.mark.parametrize("patch", [(3, 5), 0])
def test_oracle_value_and_gradient_against_autograd_on_the_float64_definition(patch):
    n, c, h, w = 2, 8, 6, 10
    fa, fb = O.features(1, n, h, w, c).astype(np.float64), O.features(2, n, h, w, c).astype(np.float64)
    g = np.array([0.75, -1.5])
    ph, pw = O.patch_of(h, w, patch)
    ta = torch.from_numpy(fa).requires_grad_(True)
    t = _definition(ta, torch.from_numpy(fb), ph, pw)
    (t * torch.from_numpy(g)).sum().backward()
    want_t, want_g = t.detach().numpy(), ta.grad.numpy()
    got_t, got_g = O.layer(fa, fb, patch), O.layer_grad(fa, fb, g, patch)
    e_t = float(np.max(np.abs(got_t - want_t) / want_t))
    e_g = float(np.max(np.abs(got_g - want_g))) / float(np.max(np.abs(want_g)))
    print(f"patch {patch}: value {e_t:.3e} relative, gradient {e_g:.3e} of the largest entry")
    assert want_t.min() > 0 and e_t <= 1e-13 and e_g <= 1e-13        # float64 sums of a few hundred terms, two orders
    assert got_g.shape == fa.shape and O.gram(fa, patch).shape == (n, (h // ph) * (w // pw), c, c)


def test_images_do_not_mix_and_g_is_linear():
    fa, fb = O.features(3, 3, 6, 10, 8), O.features(4, 3, 6, 10, 8)
    g = np.array([0.5, -2.0, 1.25])
    base = O.layer_grad(fa, fb, g, (3, 5))
    for i in range(3):
        assert np.array_equal(O.layer_grad(fa[i:i + 1], fb[i:i + 1], g[i:i + 1], (3, 5))[0], base[i])
        assert np.array_equal(O.layer(fa[i:i + 1], fb[i:i + 1], (3, 5))[0], O.layer(fa, fb, (3, 5))[i])
    zero = O.layer_grad(fa, fb, np.array([g[0], 0.0, g[2]]), (3, 5))
    assert bool((zero[1] == 0).all()) and np.array_equal(zero[0], base[0])
    assert np.array_equal(O.layer_grad(fa, fb, 2.0 * g, (3, 5)), 2.0 * base)
    assert np.array_equal(O.texture([fa, fa], [fb, fb], 0), O.layer(fa, fb, 0) + O.layer(fa, fb, 0))
    assert bool((O.layer(fa, fa, (3, 5)) == 0).all())


def test_patches_round_trip():
    f = O.features(5, 2, 6, 10, 3)
    x = O.to_patches(f, 3, 5)
    assert x.shape == (2, 4, 15, 3) and np.array_equal(O.from_patches(x, 6, 10, 3, 5), f)
    assert np.array_equal(x[1, 3, 7], f[1, 3 + 1, 5 + 2])             # patch (1, 1), pixel 7 = row 1, column 2 of it


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("pesr_gram_fwd", "pesr_gram_loss", "pesr_gram_bwd")


def test_entry_points_are_declared_and_exported():
    from pesr_amd import _lib
    lib = _lib.lib()
    for name in ENTRY_POINTS + ("pesr_gram_splits", "pesr_gram_workspace_bytes", "pesr_gram_loss_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    assert all(f"int {name}(" in header for name in ENTRY_POINTS)
    assert lib.pesr_abi_version() == 20


def test_c_abi_refuses_before_anything_is_launched():
    """PESR_EINVAL / PESR_EWORKSPACE come back without a device: the pointers are never followed on the host."""
    from pesr_amd import _lib
    lib = _lib.lib()
    p, big = 0x10000, 1 << 30
    fwd = lambda N, H, W, C, ph, pw, f=p, G=p, ws=p, nb=big: lib.pesr_gram_fwd(f, G, N, H, W, C, ph, pw, ws, nb, None)
    bwd = lambda N, H, W, C, ph, pw, f=p, dg=p, g=p, gf=p: lib.pesr_gram_bwd(f, dg, g, gf, N, H, W, C, ph, pw, None)
    loss = lambda N, P, C, a=p, b=p, t=p, dg=None, ws=p, nb=big: lib.pesr_gram_loss(a, b, t, dg, N, P, C, ws, nb, None)
    for call in (fwd, bwd):
        assert call(2, 16, 16, 64, 4, 4, f=None) == -1
        assert call(0, 16, 16, 64, 4, 4) == -1 and call(-1, 16, 16, 64, 4, 4) == -1
        for c in (0, 3, 32, 96, 512):
            assert call(2, 16, 16, c, 4, 4) == -1, c
        assert call(2, 16, 16, 64, 5, 4) == -1 and call(2, 16, 16, 64, 4, 3) == -1         # a patch that does not divide
        assert call(2, 16, 16, 64, 0, 4) == -1 and call(2, 16, 16, 64, 32, 16) == -1 and call(2, 0, 16, 64, 1, 1) == -1
        assert call(2, 16, 16, 64, 4, 4, f=p + 4) == -1
    assert fwd(2, 16, 16, 64, 4, 4, G=None) == -1 and fwd(2, 16, 16, 64, 4, 4, G=p + 8) == -1
    assert bwd(2, 16, 16, 64, 4, 4, dg=None) == -1 and bwd(2, 16, 16, 64, 4, 4, g=None) == -1 and bwd(2, 16, 16, 64, 4, 4, gf=None) == -1
    assert bwd(2, 16, 16, 64, 4, 4, g=p + 4) == -1 and bwd(2, 16, 16, 64, 4, 4, gf=p + 4) == -1
    # the workspace: only a split shape needs one, and then all of it
    assert lib.pesr_gram_splits(2, 16, 16, 64, 4, 4) == 1 and lib.pesr_gram_workspace_bytes(2, 16, 16, 64, 4, 4) == 0
    s = lib.pesr_gram_splits(2, 32, 32, 64, 32, 32)
    need = lib.pesr_gram_workspace_bytes(2, 32, 32, 64, 32, 32)
    assert s > 1 and need == s * 2 * 64 * 64 * 4
    assert fwd(2, 32, 32, 64, 32, 32, nb=need - 1) == -2 and fwd(2, 32, 32, 64, 32, 32, ws=None, nb=0) == -2
    assert lib.pesr_gram_splits(2, 16, 16, 96, 4, 4) == 0 and lib.pesr_gram_splits(2, 16, 16, 64, 5, 4) == 0
    assert lib.pesr_gram_splits(16, 192, 192, 64, 192, 192) > 1 and lib.pesr_gram_splits(16, 192, 192, 64, 16, 16) == 1
    # the distance
    assert loss(2, 4, 64, a=None) == -1 and loss(2, 4, 64, b=None) == -1 and loss(2, 4, 64, t=None) == -1
    assert loss(0, 4, 64) == -1 and loss(65536, 4, 64) == -1 and loss(2, 0, 64) == -1 and loss(2, 4, 96) == -1
    assert loss(2, 4, 64, dg=p + 4) == -1 and loss(2, 4, 64, t=p + 4) == -1
    need = lib.pesr_gram_loss_workspace_bytes(2, 4, 64)
    assert need >= 16 and loss(2, 4, 64, nb=need - 1) == -2 and loss(2, 4, 64, ws=None, nb=0) == -2
    assert lib.pesr_abi_version() == 20


def test_ops_refuse_host_tensors():
    from pesr_amd import _lib, ops
    f = torch.zeros(1, 4, 4, 64)
    G = torch.zeros(1, 1, 64, 64)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.gram(f, 0)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.gram_loss(G, G, True)
    with pytest.raises(_lib.PesrHipError, match="GPU tensors"):
        ops.gram_bwd(f, G, torch.ones(1, dtype=torch.float64), 0)


def test_gram_plan_is_a_host_question():
    from pesr_amd import ops
    assert ops.gram_plan(2, 8, 8, 64, 4, 4) == {"splits": 1, "workspace_bytes": 0, "patches": 4, "pixels": 16}
    big = ops.gram_plan(16, 192, 192, 64, 192, 192)
    assert big["splits"] > 1 and big["workspace_bytes"] == big["splits"] * 16 * 64 * 64 * 4 and big["pixels"] == 192 * 192
    with pytest.raises(ValueError, match="no Gram kernel"):
        ops.gram_plan(2, 8, 8, 96, 4, 4)


# ---- 3. train.py, Trainer, the patch rule ------------------------------------------------------------------------------------------------
def test_train_flag_default_off_and_refusals(monkeypatch):
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise AssertionError("torch.cuda was initialised")
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    Tr = _load("train")
    d = Tr.build_parser().parse_args([])
    assert d.alpha_texture == 0.0 and d.texture_patch == 16
    Tr.loss_terms_of(d)
    Tr.loss_terms_of(Tr.build_parser().parse_args(["--patch_size", "10", "--phase", "pretrain"]))      # off: anything goes
    for phase in ("pretrain", "train"):
        with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture -0\.5 must be >= 0"):
            Tr.main(["--alpha_texture", "-0.5", "--phase", phase, "--synthetic", "16"])
        with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture nan must be >= 0"):
            Tr.main(["--alpha_texture", "nan", "--phase", phase, "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture 1\.0 needs --phase train"):
        Tr.main(["--alpha_texture", "1", "--phase", "pretrain", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture 0\.5: --texture_patch 16 .* = 12 \* 4 = 48: .*48 x 48, 24 x 24, "
                                         r"12 x 12; --texture_patch 0 "):
        Tr.main(["--alpha_texture", "0.5", "--patch_size", "12", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture 1\.0: --texture_patch 5 .*32 x 32, 16 x 16, 8 x 8"):
        Tr.main(["--alpha_texture", "1", "--patch_size", "8", "--texture_patch", "5", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_texture 1\.0: --texture_patch -1 "):
        Tr.main(["--alpha_texture", "1", "--texture_patch", "-1", "--synthetic", "16"])
    for ok in (["--alpha_texture", "1", "--patch_size", "48"], ["--alpha_texture", "1", "--texture_patch", "8"], ["--alpha_texture", "1", "--patch_size", "12", "--texture_patch", "0"],
               ["--alpha_texture", "1", "--patch_size", "12", "--texture_patch", "12"]):
        Tr.loss_terms_of(Tr.build_parser().parse_args(ok))
    assert not calls


def test_trainer_term_is_off_by_default_and_refuses_a_negative_weight():
    from pesr_amd.step import Trainer
    assert not Trainer(None).use_texture and not Trainer(None, alpha_texture=0.0).use_texture
    tr = Trainer(None, alpha_texture=0.25, texture_patch=0)
    assert tr.use_texture and tr.alpha_texture == 0.25 and tr.texture_patch == 0 and Trainer(None).texture_patch == 16
    with pytest.raises(ValueError, match="alpha_texture"):
        Trainer(None, alpha_texture=-1.0)
    with pytest.raises(ValueError, match="alpha_texture"):
        Trainer(None, alpha_texture=float("nan"))
    with pytest.raises(ValueError, match="texture_patch"):
        Trainer(None, alpha_texture=1.0, texture_patch=-2)


@pytest.mark.parametrize("h,w,patch,ok", [
    (192, 192, 16, True), (192, 192, 48, True), (192, 192, 32, False), (192, 192, 0, True), (192, 192, 1, True),
    (32, 32, 8, True), (32, 32, 16, False), (32, 48, 4, True), (32, 48, 8, False), (64, 32, 8, True),
    (40, 40, 16, False), (40, 40, 10, True), (40, 40, 0, True), (30, 32, 2, False), (30, 32, 0, True), (32, 32, -1, False),
])
def test_check_patch(h, w, patch, ok):
    from pesr_amd import texture
    why = texture.check_patch(h, w, patch)
    assert (why is None) == ok, why
    if ok and patch > 0:
        assert all(th % patch == 0 and tw % patch == 0 for th, tw in texture.tap_sizes(h, w))
    assert texture.TAPS == (1, 6, 11) and texture.tap_sizes(32, 48) == [(32, 48), (16, 24), (8, 12)]
