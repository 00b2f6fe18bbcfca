"""CPU: the pieces of the channel LayerNorm in front of the window attention (--wattn_norm ln, docs/modes.md section 4x) that need no
GPU - the oracle's own checks, the C ABI and its refusals, the modules' and the Generator's refusals, the parameter order, seeded
construction, the state_dict helper, train.py's refusals and the state file's flag."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layernorm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"num_channels": 64, "depth": 4, "res_scale": 0.1}
ON = dict(OPT, wattn_every=2, wattn_dim=64)
LN = dict(ON, wattn_norm="ln")
KERNEL_CASES = [(1, 16), (33, 20), (7, 48), (306, 64), (65, 256), (65, 384), (5, 1024)]


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_ln_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _seeded(opt):
    from pesr_amd.model import Generator
    torch.manual_seed(0)
    return Generator(opt)


# ---- the oracle checks itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(33, 20), (7, 48), (65, 256)], ids=str)
def test_oracle_equals_torch_layer_norm_and_its_autograd(case):
    P, C = case
    c = O.case(P, C)
    t = [torch.as_tensor(c[k]).double().requires_grad_(True) for k in ("x", "gamma", "beta")]
    y = F.layer_norm(t[0], (C,), t[1], t[2], eps=O.EPS)
    y.backward(torch.as_tensor(c["dy"]).double())
    for name, got in zip(O.NAMES, (y.detach(), t[0].grad, t[1].grad, t[2].grad)):
        assert O.rel_err(got, c["want"][name]) <= 1e-12, name


@pytest.mark.parametrize("case", [(33, 20, "normal"), (7, 48, "big-mean"), (65, 256, "features"), (7, 16, "zero-rows")], ids=str)
def test_oracle_backward_formulas_equal_autograd(case):
    c = O.case(*case)
    for name, got in zip(O.NAMES[1:], O.analytic_backward(c["x"], c["gamma"], c["dy"])):
        assert O.rel_err(got, c["want"][name]) <= 1e-12, name


@pytest.mark.parametrize("case", [(65, 256), (7, 48)], ids=str)
def test_the_large_mean_cases_catch_a_one_pass_variance(case):
    """x = 1000 + n: E[x^2] - mean^2 in float32 loses the variance to cancellation and misses the kernels' tolerance by orders of
    magnitude, while the centred form in another summation order stays inside it - the cases are worth having."""
    c = O.case(*case, "big-mean")
    got = O.grads(c["x"], c["gamma"], c["beta"], c["dy"], torch.float32, fn=O.one_pass_layernorm)
    err, tol = O.rel_err(got[0], c["want"]["y"]), O.tolerance(c["ref"]["y"])
    assert err > 100 * tol, (err, tol)
    # the centred form with a lane-tree summation order (pairwise halving, as a shuffle butterfly adds)
    x = torch.as_tensor(c["x"])

    def tree(v):
        n = 1 << (v.shape[-1] - 1).bit_length()
        v = F.pad(v, (0, n - v.shape[-1]))
        while v.shape[-1] > 1:
            v = v[..., : v.shape[-1] // 2] + v[..., v.shape[-1] // 2:]
        return v
    C = x.shape[-1]
    mean = tree(x) / C
    d = x - mean
    y = d / torch.sqrt(tree(d * d) / C + np.float32(O.EPS)) * torch.as_tensor(c["gamma"]) + torch.as_tensor(c["beta"])
    assert y.dtype == torch.float32 and O.rel_err(y, c["want"]["y"]) <= tol


def test_zero_rows_give_beta_exactly():
    c = O.case(7, 16, "zero-rows")
    y = O.layernorm(torch.as_tensor(c["x"]), torch.as_tensor(c["gamma"]), torch.as_tensor(c["beta"]))
    assert torch.equal(y[::3], torch.as_tensor(c["beta"]).expand(3, 16)) and all(bool(torch.isfinite(v).all()) for v in c["want"].values())


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_new_symbols_keeps_its_version_and_refuses_before_any_launch():
    from pesr_amd import _lib
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    lib = _lib.lib()
    for n in ("pesr_layernorm_fwd", "pesr_layernorm_bwd", "pesr_layernorm_partials", "pesr_layernorm_workspace_bytes"):
        assert n in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % n, header) and hasattr(lib, n), n
    assert lib.pesr_abi_version() == 20
    p = 4096      # a dummy, 16-byte aligned address: validation comes before any device call, nothing is ever read through it
    eps = 1e-5

    def fwd(P, C, e=eps, ptrs=(p,) * 5):
        return lib.pesr_layernorm_fwd(*ptrs, P, C, e, None)

    def bwd(P, C, ptrs=(p,) * 8):
        return lib.pesr_layernorm_bwd(*ptrs, P, C, None)
    for bad in ((8, 0), (8, 2), (8, 18), (8, 1028), (8, 2048), (8, -4), (0, 64), (-1, 64)):
        assert fwd(*bad) == -1 and bwd(*bad) == -1, bad
        assert lib.pesr_layernorm_partials(*bad) == 0 and lib.pesr_layernorm_workspace_bytes(*bad) == 0, bad
    for e in (0.0, -1e-5, float("inf"), float("nan")):
        assert fwd(8, 64, e) == -1, e
    for i in range(5):
        assert fwd(8, 64, eps, tuple(None if j == i else p for j in range(5))) == -1, i
        assert fwd(8, 64, eps, tuple(p + 8 if j == i else p for j in range(5))) == -1, i
    for i in range(8):
        assert bwd(8, 64, tuple(None if j == i else p for j in range(8))) == -1, i
        assert bwd(8, 64, tuple(p + 4 if j == i else p for j in range(8))) == -1, i


def test_partial_rows_depend_on_the_shape_alone_and_size_the_workspace():
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    for P, C in KERNEL_CASES + [(36864, 256), (172890, 256), (300001, 16)]:
        rows = lib.pesr_layernorm_partials(P, C)
        assert rows == ops.layernorm_partials(P, C) and 1 <= rows <= 1024, (P, C, rows)
        assert lib.pesr_layernorm_workspace_bytes(P, C) == rows * 2 * C * 4
        assert ops.layernorm_pass_pixels(P, C) >= min(P, rows)
    # one workgroup takes 256 / G pixels at once, G the power of two that covers C / 4 up to 64; above 1024 of them the grid strides
    assert lib.pesr_layernorm_partials(1, 16) == 1 and lib.pesr_layernorm_partials(65, 16) == 2
    assert lib.pesr_layernorm_partials(65, 256) == 17 and lib.pesr_layernorm_partials(5, 1024) == 2
    assert lib.pesr_layernorm_partials(300001, 16) == 1024 and ops.layernorm_pass_pixels(300001, 16) == 1024 * 64 * 4 < 300001
    with pytest.raises(ValueError, match="C = 18"):
        ops.layernorm_partials(8, 18)
    with pytest.raises(ValueError, match="P = 0"):
        ops.layernorm_partials(0, 16)


def test_no_cpu_fallback():
    from pesr_amd import _lib, ops
    assert ops.LN_EPS == 1e-5
    x, g, b = torch.zeros(2, 3, 4, 16), torch.ones(16), torch.zeros(16)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.layernorm_fwd(x, g, b)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.layernorm_bwd(x, g, torch.zeros(24, 2), x)


# ---- the modules -------------------------------------------------------------------------------------------------------------------------
def test_channel_layernorm_starts_as_the_identity_scale_and_draws_nothing():
    from pesr_amd.model.basic import ChannelLayerNorm
    torch.manual_seed(5)
    before = torch.random.get_rng_state()
    m = ChannelLayerNorm(64)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert torch.equal(m.weight, torch.ones(64)) and torch.equal(m.bias, torch.zeros(64))
    assert list(m.state_dict()) == ["weight", "bias"] and m.weight.requires_grad and m.bias.requires_grad
    for bad in (0, 2, 18, 1028):
        with pytest.raises(ValueError, match="C = %d" % bad):
            ChannelLayerNorm(bad)


def test_block_refuses_an_unknown_norm_and_keeps_its_parameter_order():
    from pesr_amd.model.basic import ChannelLayerNorm, WindowAttention
    for bad in ("bn", "none", "LN", True):
        with pytest.raises(ValueError, match="norm"):
            WindowAttention(64, 64, norm=bad)
    torch.manual_seed(3)
    plain = WindowAttention(64, 64, shift=4)
    torch.manual_seed(3)
    m = WindowAttention(64, 64, shift=4, norm="ln")
    assert not hasattr(plain, "norm") and isinstance(m.norm, ChannelLayerNorm)
    assert [k for k, _ in plain.named_parameters()] == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"]
    assert [k for k, _ in m.named_parameters()] == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "norm.weight", "norm.bias"]
    assert list(m.state_dict()) == [k for k, _ in m.named_parameters()]
    for k, v in plain.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert "norm=ln" in m.extra_repr() and "norm" not in plain.extra_repr()


def test_generator_refuses_bad_arguments_naming_them():
    from pesr_amd.model import Generator
    with pytest.raises(ValueError, match="wattn_norm"):
        Generator(dict(ON, wattn_norm="bn"))
    with pytest.raises(ValueError, match="wattn_norm = 'ln' without wattn_every"):
        Generator(dict(OPT, wattn_norm="ln"))
    with pytest.raises(ValueError, match="wattn_norm = 'ln' without wattn_every"):
        Generator(dict(OPT, wattn_every=0, wattn_norm="ln"))
    for off in (None, "none"):
        g = Generator(dict(ON, wattn_norm=off))
        assert not any(".norm." in k for k in g.state_dict())
    assert not hasattr(Generator(dict(OPT, wattn_norm="none")), "wattn")


def test_ln_adds_its_keys_after_each_block_and_leaves_every_shared_tensor():
    off, on = _seeded(ON), _seeded(LN)
    a, b = off.state_dict(), on.state_dict()
    extra = [f"wattn.{i}.norm.{p}" for i in (1, 3) for p in ("weight", "bias")]
    assert sorted(b) == sorted(list(a) + extra)
    assert [k for k in b if k.startswith("wattn.1.")] == [f"wattn.1.{m}.{p}" for m in ("qkv", "proj", "norm") for p in ("weight", "bias")]
    assert [k for k in b if not k.startswith("wattn.")] == [k for k in a if not k.startswith("wattn.")]
    for k in a:                              # bit-equal initial values for every parameter the two share
        assert torch.equal(a[k], b[k]), k
    for k in extra:
        assert torch.equal(b[k], torch.ones(64) if k.endswith("weight") else torch.zeros(64)), k
    assert on.opt["wattn_norm"] == "ln"                  # (what the EMA Generator is built from)
    assert len(list(on.parameters())) == len(list(off.parameters())) + 4
    # the spelled-out default is today's Generator
    c = _seeded(dict(ON, wattn_norm="none")).state_dict()
    assert list(c) == list(a) and all(torch.equal(a[k], c[k]) for k in a)


def test_wattn_norm_of_state_dict():
    from pesr_amd.model import wattn_norm_of_state_dict, wattn_of_state_dict
    plain, off, on = _seeded(OPT).state_dict(), _seeded(ON).state_dict(), _seeded(LN).state_dict()
    assert wattn_norm_of_state_dict(plain) == "none" and wattn_norm_of_state_dict(off) == "none" and wattn_norm_of_state_dict(on) == "ln"
    assert wattn_norm_of_state_dict({"module." + k: v for k, v in on.items()}) == "ln"
    assert wattn_norm_of_state_dict({"module." + k: v for k, v in off.items()}) == "none"
    assert wattn_of_state_dict(on) == wattn_of_state_dict(off) == ((1, 3), 64)          # (its results are what they were)
    mixed = {k: v for k, v in on.items() if not k.startswith("wattn.3.norm.")}
    with pytest.raises(ValueError, match=r"\['1'\] have a norm, \['3'\] have none"):
        wattn_norm_of_state_dict(mixed)
    with pytest.raises(ValueError, match=r"wattn.3.norm.weight \(32,\)"):
        wattn_norm_of_state_dict({**on, "wattn.3.norm.weight": torch.ones(32)})
    with pytest.raises(ValueError, match=r"wattn.1.norm.bias \(64, 1\)"):
        wattn_norm_of_state_dict({**on, "wattn.1.norm.bias": torch.zeros(64, 1)})
    with pytest.raises(ValueError, match="wattn.1.norm.bias None"):
        wattn_norm_of_state_dict({k: v for k, v in on.items() if k != "wattn.1.norm.bias"})


def test_loader_of_test_py_reads_the_norm_from_the_checkpoint(tmp_path):
    from pesr_amd.model.basic import ChannelLayerNorm
    T = _entry("test")
    off, on = _seeded(ON).state_dict(), _seeded(LN).state_dict()
    on = {k: (v + 0.25 if ".norm." in k else v) for k, v in on.items()}             # (not the initial values: they have to be loaded)
    for name, sd, want in (("off", off, 0), ("on", on, 2), ("wrapped", {"module." + k: v for k, v in on.items()}, 2)):
        path = str(tmp_path / (name + ".pt"))
        torch.save(sd, path)
        G = T.load_generator(dict(OPT), path, 4)
        assert sum(isinstance(m, ChannelLayerNorm) for m in G.modules()) == want, name
        ref = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        got = G.state_dict()
        assert sorted(got) == sorted(ref) and all(torch.equal(got[k], ref[k]) for k in ref)
    path = str(tmp_path / "mixed.pt")
    torch.save({k: v for k, v in on.items() if not k.startswith("wattn.3.norm.")}, path)
    with pytest.raises(SystemExit) as e:
        T.load_generator(dict(OPT), path, 4)
    assert "test.py: " + path in str(e.value) and "have none" in str(e.value)


# ---- train.py ----------------------------------------------------------------------------------------------------------------------------
def test_train_py_flag_and_refusals():
    T = _entry("train")
    base = ["--num_channels", "64", "--num_blocks", "4"]
    args = lambda *a: T.build_parser().parse_args(base + list(a))
    assert args().wattn_norm == "none" and T.wattn_norm_of(args()) is None
    assert T.wattn_norm_of(args("--wattn_every", "2")) is None
    assert T.wattn_norm_of(args("--wattn_every", "2", "--wattn_norm", "ln")) == "ln"
    for a in (("--wattn_norm", "ln"), ("--wattn_norm", "ln", "--wattn_every", "0"), ("--wattn_norm", "ln", "--wattn_dim", "64")):
        with pytest.raises(SystemExit) as e:
            T.wattn_norm_of(args(*a))
        assert "--wattn_norm ln" in str(e.value) and "--wattn_every" in str(e.value)
    with pytest.raises(SystemExit):
        args("--wattn_norm", "bn")                          # argparse's choices


def test_train_py_refuses_ln_without_blocks_before_any_device_is_touched(monkeypatch):
    T = _entry("train")

    def no_device(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "device_count", no_device)
    with pytest.raises(SystemExit) as e:
        T.main(["--phase", "pretrain", "--synthetic", "4", "--wattn_norm", "ln"])
    assert "--wattn_norm ln" in str(e.value)


def test_pretrained_model_with_another_norm_names_both_sides():
    T = _entry("train")
    off, on = _seeded(ON).state_dict(), _seeded(LN).state_dict()
    base = ["--num_channels", "64", "--num_blocks", "4", "--wattn_every", "2", "--wattn_dim", "64"]
    args = lambda *a: T.build_parser().parse_args(base + list(a))
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn_norm(on, args(), "g.pt")
    assert "--pretrained_model g.pt" in str(e.value) and "norm 'ln'" in str(e.value) and "--wattn_norm none" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn_norm(off, args("--wattn_norm", "ln"), "g.pt")
    assert "norm 'none'" in str(e.value) and "--wattn_norm ln" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn_norm({k: v for k, v in on.items() if not k.startswith("wattn.3.norm.")}, args("--wattn_norm", "ln"), "g.pt")
    assert "--pretrained_model g.pt" in str(e.value) and "have none" in str(e.value)
    assert T.check_pretrained_wattn_norm(off, args(), "g.pt") is off
    assert T.check_pretrained_wattn_norm(on, args("--wattn_norm", "ln"), "g.pt") is on
    # the blocks' own check does not mind the norm's keys
    assert T.check_pretrained_wattn(on, args("--wattn_norm", "ln"), "g.pt") is on


def test_state_file_flag():
    from pesr_amd import checkpoint
    T = _entry("train")
    args = lambda *a: T.build_parser().parse_args(["--num_channels", "128", "--num_blocks", "4", "--wattn_every", "2", *a])
    assert "wattn_norm" in checkpoint.SHAPE_FLAGS and checkpoint._LATER_FLAGS["wattn_norm"] == "none" and checkpoint.FORMAT == 1
    assert checkpoint.shape_flags(args())["wattn_norm"] == "none"
    assert checkpoint.shape_flags(args("--wattn_norm", "ln"))["wattn_norm"] == "ln"
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(args("--wattn_norm", "ln"))}
    checkpoint.check_flags(saved, args("--wattn_norm", "ln"))
    with pytest.raises(SystemExit, match="--wattn_norm = 'ln'"):
        checkpoint.check_flags(saved, args())
    # a state written before the flag existed: no such key, loads as none
    old = {"format": checkpoint.FORMAT, "flags": {k: v for k, v in checkpoint.shape_flags(args()).items() if k != "wattn_norm"}}
    checkpoint.check_flags(old, args())
    checkpoint.check_flags(old, args("--wattn_norm", "none"))
    with pytest.raises(SystemExit, match="--wattn_norm = 'none'"):
        checkpoint.check_flags(old, args("--wattn_norm", "ln"))
