"""CPU: the pieces of the Generator's window self-attention blocks (--wattn_every, docs/modes.md section 4w) that need no GPU - the
oracle's own checks, the flags and their refusals, seeded construction with the option off and on, the state_dict helper, the state
file's flag, the tiling line, the width question of the routed 3 x 3 path and the C ABI."""
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import window_attention_oracle as O
from helpers import gen_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"num_channels": 64, "depth": 4, "res_scale": 0.1}
ON = dict(OPT, wattn_every=2, wattn_dim=64)
KERNEL_CASES = [(1, 8, 8, 32, 0), (1, 8, 8, 32, 4), (2, 9, 17, 64, 0), (2, 9, 17, 64, 4), (1, 13, 5, 160, 4), (2, 16, 24, 128, 4),
                (1, 3, 40, 32, 0)]


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_wa_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _seeded(opt):
    from pesr_amd.model import Generator
    torch.manual_seed(0)
    return Generator(opt)


# ---- the oracle checks itself ------------------------------------------------------------------------------------------------------------
def test_oracle_windows_partition_the_image():
    shapes = {(H, W, s) for _, H, W, _, s in KERNEL_CASES} | {(1, 1, 0), (1, 1, 4), (16, 16, 0), (16, 16, 4), (12, 20, 0), (12, 20, 4),
                                                              (13, 9, 0), (13, 9, 4), (7, 23, 7)}
    for H, W, s in sorted(shapes):
        assert bool((O.query_counts(H, W, s) == 1).all()), (H, W, s)
        assert len(O.windows(H, W, s)) == -(-(H + s) // 8) * -(-(W + s) // 8)


def test_oracle_equals_scaled_dot_product_attention_on_whole_windows():
    N, H, W, D = 2, 16, 24, 64
    qkv = torch.as_tensor(O.normal_like((N, H, W, 3 * D), 5)).double()
    got = O.attention(qkv, 0)
    # [N, H/8, 8, W/8, 8, 3, heads, 32] -> [N, H/8, W/8, heads, 64 tokens, 32] per q, k, v
    t = qkv.reshape(N, H // 8, 8, W // 8, 8, 3, D // 32, 32).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, N, H // 8, W // 8, D // 32, 64, 32)
    o = F.scaled_dot_product_attention(t[0], t[1], t[2])          # (its default scale is 1 / sqrt(32))
    want = o.reshape(N, H // 8, W // 8, D // 32, 8, 8, 32).permute(0, 1, 4, 2, 5, 3, 6).reshape(N, H, W, D)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", [(2, 9, 17, 64, 4), (1, 13, 5, 160, 4), (1, 8, 8, 32, 0)], ids=str)
def test_oracle_backward_formulas_equal_autograd(case):
    N, H, W, D, s = case
    c = O.case(*case)
    err = float((O.analytic_backward(c["qkv"], c["dout"], s) - c["dqkv"]).abs().max())
    assert err <= 1e-10, err


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------
def test_train_flags_exist_with_defaults():
    T = _entry("train")
    p = T.build_parser()
    a = p.parse_args([])
    assert a.wattn_every == 0 and a.wattn_dim == 0 and T.wattn_of(a) == (0, 0)
    a = p.parse_args(["--wattn_every", "8", "--wattn_dim", "128"])
    assert (a.wattn_every, a.wattn_dim) == (8, 128) and T.wattn_of(a) == (8, 128)
    assert T.wattn_of(p.parse_args(["--wattn_every", "8"])) == (8, 128)            # 0: --num_channels / 2 of the default 256
    assert T.wattn_of(p.parse_args(["--wattn_dim", "48"])) == (0, 0)               # (a width nobody uses is nobody's business)


@pytest.mark.parametrize("argv, what", [
    (["--wattn_every", "-1"], ["--wattn_every"]),
    (["--wattn_every", "3", "--num_blocks", "2"], ["--wattn_every", "--num_blocks"]),
    (["--wattn_every", "1", "--wattn_dim", "48"], ["--wattn_dim"]),
    (["--wattn_every", "1", "--wattn_dim", "-64"], ["--wattn_dim"]),
    (["--wattn_every", "1", "--wattn_dim", "2048"], ["--wattn_dim"]),
    (["--wattn_every", "1", "--num_channels", "96"], ["--wattn_dim", "--num_channels / 2"]),            # the default width 48
    (["--wattn_every", "1", "--num_channels", "40", "--wattn_dim", "64"], ["--num_channels"]),
])
def test_train_refuses_before_any_device(argv, what, monkeypatch):
    T = _entry("train")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        T.main(argv + ["--synthetic", "4", "--phase", "pretrain"])
    for w in what:
        assert w in str(e.value), str(e.value)


# ---- module and Generator ------------------------------------------------------------------------------------------------------------------
def test_module_refuses_bad_arguments_naming_them():
    from pesr_amd.model.basic import WindowAttention
    for dim in (48, 0, 16, -32, 2048):
        with pytest.raises(ValueError, match="dim"):
            WindowAttention(64, dim)
    with pytest.raises(ValueError, match="n_feats"):
        WindowAttention(40, 64)
    with pytest.raises(ValueError, match="shift"):
        WindowAttention(64, 64, shift=8)
    m = WindowAttention(64, 128, shift=4)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "qkv.weight": (384, 64, 3, 3), "qkv.bias": (384,), "proj.weight": (64, 128, 3, 3), "proj.bias": (64,)}
    assert list(m.state_dict()) == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"]
    # constructed in that order, initialised like every Conv
    torch.manual_seed(3)
    m = WindowAttention(64, 64)
    torch.manual_seed(3)
    a, b = torch.nn.Conv2d(64, 192, 3, padding=1), torch.nn.Conv2d(64, 64, 3, padding=1)
    assert torch.equal(m.qkv.weight, a.weight) and torch.equal(m.qkv.bias, a.bias)
    assert torch.equal(m.proj.weight, b.weight) and torch.equal(m.proj.bias, b.bias)


def test_generator_refuses_bad_arguments_naming_them():
    from pesr_amd.model import Generator
    with pytest.raises(ValueError, match="wattn_every"):
        Generator(dict(OPT, wattn_every=5))
    with pytest.raises(ValueError, match="wattn_every"):
        Generator(dict(OPT, wattn_every=-1))
    with pytest.raises(ValueError, match="dim"):
        Generator(dict(OPT, wattn_every=1, wattn_dim=48))
    with pytest.raises(ValueError, match="dim"):
        Generator(dict(OPT, num_channels=96, wattn_every=1))               # the default 96 / 2 = 48 is no multiple of the head width
    assert [m.dim for m in Generator(dict(OPT, wattn_every=2)).wattn.values()] == [32, 32]       # the default: num_channels / 2


def test_off_is_todays_generator_bit_for_bit():
    ref = gen_sd(64, 4, 0)
    for opt in (OPT, dict(OPT, wattn_every=0), dict(OPT, wattn_every=0, wattn_dim=64)):
        g = _seeded(opt)
        assert not hasattr(g, "wattn")
        sd = g.state_dict()
        assert list(sd) == list(ref) and all(sd[k].shape == ref[k].shape for k in ref)
        g.load_state_dict(ref)
        assert all(torch.equal(g.state_dict()[k], ref[k]) for k in ref)
    a, b = _seeded(OPT).state_dict(), _seeded(dict(OPT, wattn_every=0)).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_on_adds_its_keys_last_and_leaves_every_other_tensor():
    base, on = _seeded(OPT).state_dict(), _seeded(ON).state_dict()
    extra = [f"wattn.{i}.{m}.{p}" for i in (1, 3) for m in ("qkv", "proj") for p in ("weight", "bias")]
    assert list(on) == list(base) + extra
    for k in base:
        assert torch.equal(on[k], base[k]), k
    assert on["wattn.1.qkv.weight"].shape == (192, 64, 3, 3) and on["wattn.3.proj.weight"].shape == (64, 64, 3, 3)
    g = _seeded(ON)
    assert [(k, m.shift, m.dim) for k, m in g.wattn.items()] == [("1", 0, 64), ("3", 4, 64)]
    assert g.opt["wattn_every"] == 2 and g.opt["wattn_dim"] == 64             # (what the EMA Generator is built from)
    every1 = _seeded(dict(OPT, wattn_every=1, wattn_dim=128))
    assert [(k, m.shift) for k, m in every1.wattn.items()] == [("0", 0), ("1", 4), ("2", 0), ("3", 4)]
    assert list(_seeded(dict(OPT, wattn_every=3, wattn_dim=64)).wattn) == ["2"]
    # together with channel attention: the blocks' own keys stay inside body, these stay last
    both = _seeded(dict(ON, attention="ca", ca_reduction=4)).state_dict()
    assert list(both)[-8:] == extra and "body.0.ca.squeeze.weight" in both


def test_wattn_of_state_dict_round_trips():
    from pesr_amd.model import wattn_of_state_dict
    plain, on = _seeded(OPT).state_dict(), _seeded(ON).state_dict()
    assert wattn_of_state_dict(plain) == ((), 0)
    assert wattn_of_state_dict(on) == ((1, 3), 64)
    assert wattn_of_state_dict({"module." + k: v for k, v in on.items()}) == ((1, 3), 64)
    assert wattn_of_state_dict({"module." + k: v for k, v in plain.items()}) == ((), 0)
    assert wattn_of_state_dict(_seeded(dict(OPT, depth=12, wattn_every=1, wattn_dim=128)).state_dict()) == (tuple(range(12)), 128)
    with pytest.raises(ValueError, match="wattn.1.qkv.weight"):
        wattn_of_state_dict({"wattn.1.qkv.weight": torch.zeros(100, 64, 3, 3), "wattn.1.proj.weight": torch.zeros(64, 33, 3, 3)})
    with pytest.raises(ValueError, match="wattn"):
        wattn_of_state_dict({"wattn.1.qkv.weight": torch.zeros(192, 64, 3, 3)})
    with pytest.raises(ValueError, match="widths"):
        wattn_of_state_dict({**on, "wattn.3.qkv.weight": torch.zeros(384, 64, 3, 3), "wattn.3.proj.weight": torch.zeros(64, 128, 3, 3)})


def test_loader_of_test_py_reads_the_blocks_from_the_checkpoint(tmp_path):
    T = _entry("test")
    plain, on = _seeded(OPT).state_dict(), _seeded(ON).state_dict()
    for name, sd, want in (("plain", plain, []), ("on", on, ["1", "3"]), ("wrapped", {"module." + k: v for k, v in on.items()}, ["1", "3"])):
        path = str(tmp_path / (name + ".pt"))
        torch.save(sd, path)
        G = T.load_generator(dict(OPT), path, 4)
        assert list(getattr(G, "wattn", {})) == want and T.has_wattn(G) == bool(want), name
        ref = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        got = G.state_dict()
        assert sorted(got) == sorted(ref) and all(torch.equal(got[k], ref[k]) for k in ref)


def test_loader_of_test_py_refuses_blocks_in_other_places_by_name(tmp_path):
    """Positions that no --wattn_every gives for this depth: a SystemExit naming the file, not a ValueError or a key dump."""
    T = _entry("test")
    on = _seeded(ON).state_dict()
    moved = {k.replace("wattn.1.", "wattn.2."): v for k, v in on.items()}                    # blocks after 2 and 3
    deeper = _seeded(dict(OPT, depth=8, wattn_every=6, wattn_dim=64)).state_dict()              # a block after 5: beyond four blocks
    for name, sd, what in (("moved", moved, "[2, 3]"), ("deeper", deeper, "[5]")):
        path = str(tmp_path / (name + ".pt"))
        torch.save({k: v for k, v in sd.items() if not k.startswith("body.") or int(k.split(".")[1]) <= 4}, path)
        with pytest.raises(SystemExit) as e:
            T.load_generator(dict(OPT), path, 4)
        assert "test.py: " + path in str(e.value) and what in str(e.value) and "--num_blocks 4" in str(e.value), str(e.value)


def test_pretrained_model_with_other_blocks_names_both_sides():
    T = _entry("train")
    plain, on = _seeded(OPT).state_dict(), _seeded(ON).state_dict()
    base = ["--num_channels", "64", "--num_blocks", "4"]
    args = lambda *a: T.build_parser().parse_args(base + list(a))
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn(on, args(), "g.pt")
    assert "--pretrained_model g.pt" in str(e.value) and "[1, 3]" in str(e.value) and "no window-attention blocks" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn(plain, args("--wattn_every", "2", "--wattn_dim", "64"), "g.pt")
    assert "--wattn_every 2" in str(e.value) and "no window-attention blocks" in str(e.value) and "[1, 3]" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn(on, args("--wattn_every", "1", "--wattn_dim", "64"), "g.pt")
    assert "[1, 3]" in str(e.value) and "[0, 1, 2, 3]" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_wattn(on, args("--wattn_every", "2", "--wattn_dim", "128"), "g.pt")
    assert "width 64" in str(e.value) and "width 128" in str(e.value)
    assert T.check_pretrained_wattn(plain, args(), "g.pt") is plain
    assert T.check_pretrained_wattn(on, args("--wattn_every", "2", "--wattn_dim", "64"), "g.pt") is on


def test_state_file_flag():
    from pesr_amd import checkpoint
    T = _entry("train")
    args = lambda *a: T.build_parser().parse_args(["--num_channels", "128", "--num_blocks", "4", *a])
    assert "wattn" in checkpoint.SHAPE_FLAGS and checkpoint.FORMAT == 1
    assert checkpoint.shape_flags(args())["wattn"] == 0
    assert checkpoint.shape_flags(args("--wattn_dim", "64"))["wattn"] == 0
    assert checkpoint.shape_flags(args("--wattn_every", "2"))["wattn"] == (2, 64)
    assert checkpoint.shape_flags(args("--wattn_every", "2", "--wattn_dim", "128"))["wattn"] == (2, 128)
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(args("--wattn_every", "2"))}
    checkpoint.check_flags(saved, args("--wattn_every", "2"))
    checkpoint.check_flags(saved, args("--wattn_every", "2", "--wattn_dim", "64"))
    for other in ((), ("--wattn_every", "1"), ("--wattn_every", "2", "--wattn_dim", "128")):
        with pytest.raises(SystemExit, match="--wattn_every"):
            checkpoint.check_flags(saved, args(*other))
    # a state written before the flag existed: no such key, counts as off
    old = {"format": checkpoint.FORMAT, "flags": {k: v for k, v in checkpoint.shape_flags(args()).items() if k != "wattn"}}
    checkpoint.check_flags(old, args())
    with pytest.raises(SystemExit, match="--wattn_every"):
        checkpoint.check_flags(old, args("--wattn_every", "2"))


def test_tiling_line_has_its_own_sentence():
    from pesr_amd import tile
    exact = tile.receptive_halo(32, 4)
    for halo in (8, exact):
        for attention in (False, True):
            plain = tile.describe(32, halo, exact, attention=attention)
            assert "window" not in plain and plain == tile.describe(32, halo, exact, attention=attention, wattn=False)
            line = tile.describe(32, halo, exact, attention=attention, wattn=True)
            assert line.startswith(plain) and "window-attention" in line[len(plain):] and "APPROXIMATION" in line[len(plain):]
    assert "equals" in tile.describe(32, exact, exact) and "APPROXIMATION" not in tile.describe(32, exact, exact)


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_the_routed_3x3_path_takes_multiples_of_16_in_all_three_passes():
    """The width question, settled by asking the library (no device: refusals come before any device call, acceptance is asked of the
    kernels' dry planner): a conv's forward wants Cin % 16 == 0 and pads Cout to its tile itself, its input gradient is the same kernel
    with the two exchanged, so Cout % 16 == 0, the weight gradient wants multiples of 4.  A legal attention width (a multiple of 32) and
    its threefold are multiples of 16, so the constructor has only n_feats left to refuse."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    fwd = lambda cin, cout: lib.pesr_conv3x3_fwd(None, None, None, None, None, None, 2, 12, 20, cin, cout, 1, 1.0, 0, 0.0, 0, None, 0, None)
    dgrad = lambda cin, cout: lib.pesr_conv3x3_dgrad(None, None, None, None, None, 2, 12, 20, cin, cout, 1, 1.0, 0, None, 0, None)
    for c in (8, 24, 40, 72):
        assert fwd(c, 64) == -1 and dgrad(64, c) == -1, c                  # a conv from c channels; the input gradient of a conv to c
    assert lib.pesr_conv3x3_wgrad_workspace_bytes(2, 12, 20, 64, 66, 1, 0) == 0
    # the projections of dim = 32, 64, 128 on 16, 64 and 256 features: planned forward (0) and backward (1), and a weight-gradient plan
    for n_feats, dim in ((64, 32), (64, 64), (16, 64), (256, 128)):
        for cin, cout in ((n_feats, 3 * dim), (dim, n_feats)):
            assert lib.pesr_conv3x3_bn_rows(1, 2, 12, 20, cin, cout, 1) > 0, (cin, cout)
            assert lib.pesr_conv3x3_wgrad_workspace_bytes(2, 12, 20, cin, cout, 1, 0) > 0, (cin, cout)
        assert lib.pesr_conv3x3_bn_rows(0, 2, 12, 20, dim, n_feats, 1) > 0
    assert [c for c in range(1, 70) if ops.routed_3x3_width_ok(c)] == [16, 32, 48, 64]
    assert ops.wattn_check_widths("t", 256, 128) == 4 and ops.wattn_check_widths("t", 64, 32) == 1 and ops.wattn_check_widths("t", 16, 64) == 2
    for n_feats, dim, name in ((256, 16, "dim"), (256, 48, "dim"), (256, 100, "dim"), (256, 1056, "dim"), (40, 64, "n_feats"), (8, 64, "n_feats")):
        with pytest.raises(ValueError, match=name):
            ops.wattn_check_widths("t", n_feats, dim)


def test_abi_has_the_new_symbols_keeps_its_version_and_refuses_before_any_launch():
    from pesr_amd import _lib
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    lib = _lib.lib()
    for n in ("pesr_window_attention_fwd", "pesr_window_attention_bwd"):
        assert n in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % n, header) and hasattr(lib, n), n
        assert _lib.SIGNATURES[n][1][-1] is _lib._P                     # the stream comes last
    assert lib.pesr_abi_version() == 20
    p = 4096      # a dummy, 16-byte aligned address: validation comes before any device call, nothing is ever read through it
    fwd = lambda N, H, W, D, s, a=p, b=p: lib.pesr_window_attention_fwd(a, b, N, H, W, D, s, None)
    bwd = lambda N, H, W, D, s, a=p, b=p, c=p: lib.pesr_window_attention_bwd(a, b, c, N, H, W, D, s, None)
    for f in (fwd, bwd):
        for bad in ((1, 8, 8, 16, 0), (1, 8, 8, 0, 0), (1, 8, 8, 48, 0), (1, 8, 8, 1056, 0), (1, 8, 8, 32, -1), (1, 8, 8, 32, 8),
                    (0, 8, 8, 32, 0), (1, 0, 8, 32, 0), (1, 8, 0, 32, 0), (-1, 8, 8, 32, 0)):
            assert f(*bad) == -1, bad
        assert f(1, 8, 8, 32, 0, None) == -1 and f(1, 8, 8, 32, 0, p, None) == -1 and f(1, 8, 8, 32, 0, p + 4) == -1
    assert bwd(1, 8, 8, 32, 0, p, p, None) == -1
    assert fwd(1 << 15, 1 << 12, 1 << 12, 32, 0) == -1               # more windows than a grid has workgroups


def test_no_cpu_fallback_and_refusals_name_the_argument():
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.window_attention_fwd(torch.zeros(1, 8, 8, 96))
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.window_attention_bwd(torch.zeros(1, 8, 8, 96), torch.zeros(1, 8, 8, 32))
