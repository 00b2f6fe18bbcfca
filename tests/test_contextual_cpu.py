"""CPU: the contextual loss (docs/modes.md section 4r) - the restatement's closed-form gradient (tests/contextual_oracle.py) against
torch.autograd on a float64 statement of the definition, the conditions that the GPU cases' inputs must meet (asserted from the oracle
alone), the refusals of the C entry points, of the ops, of train.py --alpha_cx and of the Trainer, and the size rule."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import contextual_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2
# (C, H, W, regime, seed) of tests/test_contextual_gpu.py; its last case is found by asking ops.cx_plan and is (64, 5, 13): P = 65
GPU_CASES = [(64, 4, 4, "matched", 100), (64, 5, 7, "unmatched", 110), (128, 8, 8, "matched", 120), (256, 8, 9, "unmatched", 130),
             (256, 16, 16, "unmatched", 141), (128, 5, 7, "unmatched", 166), (64, 5, 13, "matched", 151)]


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_contextual_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _definition(x, y, h):
    """The definition with torch ops in float64, image by image, independent of the oracle's batched statement: [N]"""
    n, c = x.shape[0], x.shape[-1]
    out = []
    for i in range(n):
        xs, ys = x[i].reshape(-1, c), y[i].reshape(-1, c)
        mu = ys.mean(0)
        xb, yb = xs - mu, ys - mu
        xh = xb / torch.sqrt((xb ** 2).sum(1, keepdim=True) + 1e-12)
        yh = yb / torch.sqrt((yb ** 2).sum(1, keepdim=True) + 1e-12)
        d = (1 - xh @ yh.t()) / 2
        w = torch.exp((1 - d / (d.min(1, keepdim=True).values + 1e-5)) / h)
        cij = w / w.sum(1, keepdim=True)
        out.append(-torch.log(cij.max(0).values.mean()))
    return torch.stack(out)


# ---- 1. the gradient formula is the derivative of the definition ----------------------------------------------------------------------
@pytest.mark.parametrize("regime,h", [("matched", 0.5), ("unmatched", 0.5), ("unmatched", 0.25)])
def test_oracle_value_and_gradient_against_autograd_on_the_float64_definition(regime, h):
    fa, fb = O.features(1, N, 5, 6, 16, regime)
    g = np.array([0.75, -1.5])
    x = torch.tensor(fa.astype(np.float64), requires_grad=True)
    L = _definition(x, torch.tensor(fb.astype(np.float64)), h)
    (L * torch.from_numpy(g)).sum().backward()
    got = O.grad(fa, fb, g, h)
    e_l = float((got["L"] - L.detach()).abs().max() / L.detach().abs().max())
    e_g = float(np.max(np.abs(got["gf"] - x.grad.numpy()))) / float(np.max(np.abs(x.grad.numpy())))
    print(f"{regime}, h {h}: value {e_l:.3e} relative, gradient {e_g:.3e} of the largest entry")
    assert float(L.detach().min()) > 0 and e_l <= 1e-12 and e_g <= 1e-12
    assert got["gf"].shape == fa.shape and tuple(got["E"].shape) == (N, 30, 30) and tuple(got["gxh"].shape) == (N, 30, 16)
    assert np.array_equal(O.loss(fa, fb, h), got["L"].numpy())


def test_selections_given_as_arguments_are_used():
    fa, fb = O.features(2, N, 4, 4, 8, "unmatched")
    s = O.stages(fa, fb)
    same = O.stages(fa, fb, a=s["a"].numpy(), b=s["b"].numpy())
    assert torch.equal(same["L"], s["L"])
    other = O.stages(fa, fb, a=np.zeros((N, 16), dtype=np.int64))
    assert float(other["CX"].max()) < float(s["CX"].min())           # not the arg max: a smaller sum


def test_images_do_not_mix_and_g_is_linear():
    fa, fb = O.features(3, 3, 4, 5, 8, "unmatched")
    g = np.array([0.5, -2.0, 1.25])
    base = O.grad(fa, fb, g)
    for i in range(3):
        one = O.grad(fa[i:i + 1], fb[i:i + 1], g[i:i + 1])
        assert np.array_equal(one["gf"][0], base["gf"][i]) and float(one["L"][0]) == float(base["L"][i])
    zero = O.grad(fa, fb, np.array([g[0], 0.0, g[2]]))["gf"]
    assert bool((zero[1] == 0).all()) and np.array_equal(zero[0], base["gf"][0])
    assert np.array_equal(O.grad(fa, fb, 2.0 * g)["gf"], 2.0 * base["gf"])
    fb2 = fb.copy()
    fb2[0] = fa[0]
    assert O.loss(fa, fb2)[1] == O.loss(fa, fb)[1]


# ---- 2. what the GPU cases' inputs must be, from the oracle alone ------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w,regime,seed", GPU_CASES)
def test_conditions_on_the_gpu_cases_inputs(c, h, w, regime, seed):
    """The selections of an fp32 run can be compared exactly only when no two candidates are closer than the fp32 error: in every row
    the two smallest d differ by >= 1e-5, in every column the two largest c by >= 1e-4 of the largest; min m >= 0.03 keeps the
    exponent's condition number 1 / ((m + eps) h) below 67; 0 < CX < 1; the unmatched inputs have many-to-one arg maxima."""
    fa, fb = O.features(seed, N, h, w, c, regime)
    assert fa.dtype == np.float32 and fa.min() == 0 and fb.min() == 0 and fa.shape == (N, h, w, c)
    s = O.stages(fa, fb)
    d2 = torch.sort(s["D"], dim=2).values
    gap_d = float((d2[:, :, 1] - d2[:, :, 0]).min())
    c2 = torch.sort(s["c"], dim=1, descending=True).values
    gap_c = float(((c2[:, 0] - c2[:, 1]) / c2[:, 0]).min())
    distinct = [len(set(s["a"][n].tolist())) for n in range(N)]
    print(f"{c} x {h} x {w} {regime}: row gap {gap_d:.2e}, column gap {gap_c:.2e}, m {float(s['m'].min()):.3f} .. {float(s['m'].max()):.3f}, "
          f"CX {s['CX'].tolist()}, L {s['L'].tolist()}, distinct arg maxima {distinct} of {h * w}")
    assert gap_d >= 1e-5 and gap_c >= 1e-4
    assert float(s["m"].min()) >= 0.03
    assert 0 < float(s["CX"].min()) and float(s["CX"].max()) < 1
    if regime == "unmatched":
        assert min(distinct) < h * w
    else:
        assert distinct == [h * w] * N and torch.equal(s["a"], s["b"])    # every point is matched to its own


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("pesr_cx_normalize", "pesr_cx_dist", "pesr_cx_fwd", "pesr_cx_bwd")
PLANNERS = ("pesr_cx_row_blocks", "pesr_cx_col_pieces", "pesr_cx_workspace_bytes", "pesr_cx_saved_bytes")


def test_entry_points_are_declared_and_exported():
    from pesr_amd import _lib
    lib = _lib.lib()
    for name in ENTRY_POINTS + PLANNERS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    assert all(f"int {name}(" in header for name in ENTRY_POINTS) and all(f" {name}(int N, int P, int C);" in header for name in PLANNERS)
    assert lib.pesr_abi_version() == 20


def test_c_abi_refuses_before_anything_is_launched():
    """PESR_EINVAL / PESR_EWORKSPACE come back without a device: the pointers are never followed on the host."""
    from pesr_amd import _lib
    lib = _lib.lib()
    p, big = 0x10000, 1 << 40
    norm = lambda N, P, C, fa=p: lib.pesr_cx_normalize(fa, p, p, p, p, p, N, P, C, None)
    dist = lambda N, P, C, xh=p: lib.pesr_cx_dist(xh, p, p, p, p, N, P, C, None)
    fwd = lambda N, P, C, D=p, h=0.5, ws=p, nb=big: lib.pesr_cx_fwd(D, p, h, p, p, p, p, p, N, P, C, ws, nb, None)
    bwd = lambda N, P, C, D=p, h=0.5, ws=p, nb=big, gL=p: lib.pesr_cx_bwd(D, p, p, p, p, p, p, gL, p, p, p, h, p, None, None, N, P, C, ws, nb, None)
    for call in (norm, dist, fwd, bwd):
        assert call(2, 16, 96) == -1 and call(2, 16, 32) == -1 and call(2, 16, 512) == -1         # C outside {64, 128, 256}
        assert call(2, 0, 64) == -1 and call(2, 4097, 64) == -1 and call(2, -1, 64) == -1          # P outside 1 .. 4096
        assert call(0, 16, 64) == -1 and call(65536, 16, 64) == -1
        assert call(2, 16, 64, None) == -1                                                      # a null pointer
    assert norm(2, 16, 64, p + 4) == -1 and dist(2, 16, 64, p + 4) == -1 and bwd(2, 16, 64, gL=p + 4) == -1
    for call in (fwd, bwd):
        assert call(2, 16, 64, h=0.0) == -1 and call(2, 16, 64, h=-1.0) == -1 and call(2, 16, 64, h=float("nan")) == -1
        need = lib.pesr_cx_workspace_bytes(2, 16, 64)
        assert need == 2 * 1 * 16 * 8 and call(2, 16, 64, nb=need - 1) == -2 and call(2, 16, 64, ws=None, nb=0) == -2
    for planner in PLANNERS:
        fn = getattr(lib, planner)
        assert fn(2, 16, 96) == 0 and fn(2, 0, 64) == 0 and fn(2, 4097, 64) == 0 and fn(2, 4096, 256) > 0
    assert lib.pesr_abi_version() == 20


def test_ops_refuse_host_tensors():
    from pesr_amd import _lib, ops
    f = torch.zeros(1, 4, 4, 64)
    x, D, v = torch.zeros(1, 16, 64), torch.zeros(1, 16, 16), torch.zeros(1, 16)
    i, g = torch.zeros(1, 16, dtype=torch.int32), torch.ones(1, dtype=torch.float64)
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        ops.cx_normalize(f, f)
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        ops.cx_dist(x, x)
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        ops.cx_fwd(D, v, 0.5, 64)
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        ops.cx_bwd(g, x, x, v, D, v, i, v, i, v, g, 0.5)
    from pesr_amd import functional as PF
    with pytest.raises(_lib.PesrHipError, match="GPU tensor"):
        PF.contextual_layer(f, f, 0.5)


def test_cx_plan_is_a_host_question():
    from pesr_amd import ops
    assert ops.cx_plan(2, 16, 64) == {"row_blocks": 1, "col_pieces": 1, "workspace_bytes": 2 * 16 * 8,
                                      "saved_bytes": 2 * 16 * (2 * 64 + 16 + 6) * 4 + 2 * 8}
    assert ops.cx_plan(2, 64, 128)["row_blocks"] == 1 and ops.cx_plan(2, 65, 128)["row_blocks"] == 2
    big = ops.cx_plan(16, 48 * 48, 256)
    assert big["row_blocks"] == 36 and big["col_pieces"] == 36 and big["workspace_bytes"] == 16 * 36 * 2304 * 8
    assert big["saved_bytes"] == 16 * 2304 * (512 + 2304 + 6) * 4 + 16 * 8          # D alone is 340 MB
    for bad in ((2, 16, 96), (2, 0, 64), (2, 4097, 64)):
        with pytest.raises(ValueError, match="no contextual kernel"):
            ops.cx_plan(*bad)


# ---- 4. train.py, Trainer, the size rule ------------------------------------------------------------------------------------------------
def test_train_flag_default_off_and_refusals(monkeypatch):
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise AssertionError("torch.cuda was initialised")
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    Tr = _load("train")
    d = Tr.build_parser().parse_args([])
    assert d.alpha_cx == 0.0 and d.cx_h == 0.5
    Tr.loss_terms_of(d)
    Tr.loss_terms_of(Tr.build_parser().parse_args(["--patch_size", "10", "--phase", "pretrain"]))      # off: anything goes
    for phase in ("pretrain", "train"):
        with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx -0\.5 must be >= 0"):
            Tr.main(["--alpha_cx", "-0.5", "--phase", phase, "--synthetic", "16"])
        with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx nan must be >= 0"):
            Tr.main(["--alpha_cx", "nan", "--phase", phase, "--synthetic", "16"])
    for h in ("0", "-0.5", "nan"):
        with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx 1\.0: --cx_h \S+ must be > 0"):
            Tr.main(["--alpha_cx", "1", "--cx_h", h, "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx 1\.0 needs --phase train"):
        Tr.main(["--alpha_cx", "1", "--phase", "pretrain", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx 0\.5: .* = 65 \* 4 = 260, a relu3_4 tap of 65 x 65: .*4225 points"):
        Tr.main(["--alpha_cx", "0.5", "--patch_size", "65", "--synthetic", "16"])
    with pytest.raises(SystemExit, match=r"^train\.py: --alpha_cx 1\.0: .* = 15 \* 2 = 30, a relu3_4 tap of 7 x 7: .*multiples of 4"):
        Tr.main(["--alpha_cx", "1", "--patch_size", "15", "--scale", "2", "--synthetic", "16"])
    for ok in (["--alpha_cx", "1"], ["--alpha_cx", "1", "--patch_size", "48"], ["--alpha_cx", "0.1", "--patch_size", "64", "--cx_h", "0.1"],
               ["--alpha_cx", "1", "--patch_size", "2", "--scale", "2"]):
        Tr.loss_terms_of(Tr.build_parser().parse_args(ok))
    assert not calls


def test_trainer_term_is_off_by_default_and_refuses_a_negative_weight():
    from pesr_amd.step import Trainer
    assert not Trainer(None).use_cx and not Trainer(None, alpha_cx=0.0).use_cx and Trainer(None).cx_h == 0.5
    tr = Trainer(None, alpha_cx=0.25, cx_h=0.1)
    assert tr.use_cx and tr.alpha_cx == 0.25 and tr.cx_h == 0.1 and not tr.use_texture
    with pytest.raises(ValueError, match="alpha_cx"):
        Trainer(None, alpha_cx=-1.0)
    with pytest.raises(ValueError, match="alpha_cx"):
        Trainer(None, alpha_cx=float("nan"))
    for h in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="cx_h"):
            Trainer(None, alpha_cx=1.0, cx_h=h)


@pytest.mark.parametrize("h,w,ok,why", [
    (192, 192, True, None), (96, 96, True, None), (256, 256, True, None), (4, 4, True, None), (32, 48, True, None),
    (1028, 1028, False, "66049 points"), (260, 256, False, "4160 points"), (30, 30, False, "multiples of 4"),
    (32, 30, False, "multiples of 4"), (2, 2, False, "multiples of 4"),
])
def test_check_size(h, w, ok, why):
    from pesr_amd import contextual
    got = contextual.check_size(h, w)
    assert (got is None) == ok, got
    if not ok:
        assert why in got
    else:
        th, tw = contextual.tap_size(h, w)
        assert (th, tw) == (h // 4, w // 4) and th * tw <= contextual.MAX_POINTS
    assert contextual.TAP == 17 and contextual.TAP_CHANNELS == 256 and contextual.MAX_POINTS == 4096


def test_vgg_refuses_taps_that_are_not_relus_in_front_of_the_tail():
    import warnings
    from pesr_amd.model.vgg import VGG
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V = VGG()
    assert V._tap_indices(False) is None and V._tap_indices(True) == (1, 6, 11) and V._tap_indices((17, 1)) == (1, 17)
    assert isinstance(V.vgg[17], torch.nn.ReLU) and V.TAIL_START == 19
    for bad in ((16,), (18,), (20,), (0,), ()):
        with pytest.raises(ValueError, match="VGG taps"):
            V._tap_indices(bad)
