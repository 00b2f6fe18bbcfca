"""CPU: the pieces of the Generator's channel attention (--attention ca, docs/modes.md section 4u) that need no GPU - the flags and
their refusals, seeded construction with the option off and on, the state_dict helper and test.py's loader, the state file's flag,
the tiling line, and the C ABI."""
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"num_channels": 16, "depth": 2, "res_scale": 0.1}


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_ca_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _seeded(opt):
    from pesr_amd.model import Generator
    torch.manual_seed(0)
    return Generator(opt)


def test_train_flags_exist_with_defaults():
    p = _entry("train").build_parser()
    a = p.parse_args([])
    assert a.attention == "none" and a.ca_reduction == 16
    a = p.parse_args(["--attention", "ca", "--ca_reduction", "8"])
    assert a.attention == "ca" and a.ca_reduction == 8
    with pytest.raises(SystemExit):
        p.parse_args(["--attention", "se"])


@pytest.mark.parametrize("argv, what", [
    (["--attention", "ca", "--ca_reduction", "0"], "--ca_reduction"),
    (["--ca_reduction", "0"], "--ca_reduction"),
    (["--attention", "ca", "--ca_reduction", "3", "--num_channels", "16"], "--ca_reduction"),
    (["--ca_reduction", "3", "--num_channels", "16"], "--ca_reduction"),
    (["--attention", "ca", "--ca_reduction", "-4", "--num_channels", "16"], "--ca_reduction"),
])
def test_train_refuses_a_bad_reduction_before_any_device(argv, what, monkeypatch):
    T = _entry("train")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        T.main(argv + ["--synthetic", "4", "--phase", "pretrain"])
    assert what in str(e.value)


def test_train_accepts_the_default_reduction_without_attention():
    """Off by default: a width the default reduction does not divide is nobody's business in a run without attention."""
    T = _entry("train")
    assert T.attention_of(T.build_parser().parse_args(["--num_channels", "24"])) == 0
    assert T.attention_of(T.build_parser().parse_args(["--num_channels", "64", "--attention", "ca", "--ca_reduction", "4"])) == 4


def test_module_refuses_shapes_naming_the_argument():
    from pesr_amd.model.basic import ChannelAttention, ResBlock
    with pytest.raises(ValueError, match="n_feats"):
        ChannelAttention(18, 4)
    with pytest.raises(ValueError, match="reduction"):
        ChannelAttention(16, 3)
    with pytest.raises(ValueError, match="reduction"):
        ChannelAttention(16, 0)
    with pytest.raises(ValueError, match="attention"):
        ResBlock(16, 3, attention="se")
    ca = ChannelAttention(16, 4)
    assert {k: tuple(v.shape) for k, v in ca.state_dict().items()} == {
        "squeeze.weight": (4, 16, 1, 1), "squeeze.bias": (4,), "excite.weight": (16, 4, 1, 1), "excite.bias": (16,)}


def test_ops_refuse_shapes_naming_the_argument():
    from pesr_amd import ops
    with pytest.raises(ValueError, match="C = 18"):
        ops.ca_pool_partials(2, 35, 18)
    with pytest.raises(ValueError, match="HW"):
        ops.ca_pool_partials(2, 0, 16)
    with pytest.raises(ValueError, match="N = 0"):
        ops.ca_pool_partials(0, 35, 16)


def test_chunk_rule_is_a_host_function():
    """The chunk rule fills the chip at the training shape and for one large image, and gives the tests a ragged last chunk."""
    from pesr_amd import ops
    assert ops.ca_pool_partials(16, 48 * 48, 256) == 72                    # 16 x 72 = 1152 workgroups of 32 pixels
    assert ops.ca_pool_partials(1, 512 * 512, 256) == 2048                 # one image: 2048 workgroups of 128 pixels
    assert ops.ca_pool_partials(2, 1, 16) == 1
    n = ops.ca_pool_partials(1, 97 * 61, 64)
    assert n == 47 and (97 * 61) % 128 != 0                                # 46 chunks of 128 pixels and one of 29


def test_off_by_default_is_todays_generator():
    a, b = _seeded(OPT), _seeded(dict(OPT, attention=None))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and not any(".ca." in k for k in sa)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    assert not hasattr(a.body[0], "ca") and "attention" not in a.opt


def test_on_adds_four_keys_per_block_after_the_blocks_convs():
    C, depth, red = 16, 2, 4
    R = C // red
    base, on = _seeded(OPT), _seeded(dict(OPT, attention="ca", ca_reduction=red))
    sb, so = base.state_dict(), on.state_dict()
    extra = [f"body.{i}.ca.{m}.{p}" for i in range(depth) for m in ("squeeze", "excite") for p in ("weight", "bias")]
    assert sorted(so) == sorted(list(sb) + extra)
    count = lambda g: sum(p.numel() for p in g.parameters())
    assert count(on) == count(base) + depth * (2 * C * R + R + C)
    assert so["body.0.ca.squeeze.weight"].shape == (R, C, 1, 1) and so["body.1.ca.excite.weight"].shape == (C, R, 1, 1)
    assert on.opt["attention"] == "ca" and on.opt["ca_reduction"] == red          # (what the EMA Generator is built from)
    # registered after `body` inside a block
    keys0 = [k for k in so if k.startswith("body.0.")]
    assert keys0.index("body.0.ca.squeeze.weight") > keys0.index("body.0.body.2.bias")
    # RNG order: block i's two convs, then its squeeze, then its excite, then block i + 1 - replayed here with the same initialisers
    torch.manual_seed(0)
    for i in range(depth):
        for j in (0, 2):
            ref = torch.nn.Conv2d(C, C, 3, padding=1)
            assert torch.equal(so[f"body.{i}.body.{j}.weight"], ref.weight.data), (i, j)
            assert torch.equal(so[f"body.{i}.body.{j}.bias"], ref.bias.data), (i, j)
        sq, ex = torch.nn.Conv2d(C, R, 1), torch.nn.Conv2d(R, C, 1)
        assert torch.equal(so[f"body.{i}.ca.squeeze.weight"], sq.weight.data) and torch.equal(so[f"body.{i}.ca.squeeze.bias"], sq.bias.data)
        assert torch.equal(so[f"body.{i}.ca.excite.weight"], ex.weight.data) and torch.equal(so[f"body.{i}.ca.excite.bias"], ex.bias.data)
    # the first block's convs are drawn before any attention parameter: they are the plain Generator's
    for j in (0, 2):
        assert torch.equal(so[f"body.0.body.{j}.weight"], sb[f"body.0.body.{j}.weight"])


def test_a_plain_checkpoint_loads_into_a_plain_generator_as_before():
    sd = _seeded(OPT).state_dict()
    g = _seeded(OPT)
    assert g.load_state_dict(sd).missing_keys == []
    with pytest.raises(RuntimeError):
        _seeded(dict(OPT, attention="ca", ca_reduction=4)).load_state_dict(sd)


def test_attention_of_state_dict_and_the_loader(tmp_path):
    from pesr_amd.model import attention_of_state_dict
    from pesr_amd.model.basic import ChannelAttention
    plain = _seeded(OPT).state_dict()
    on = _seeded(dict(OPT, attention="ca", ca_reduction=4)).state_dict()
    wrapped = {"module." + k: v for k, v in on.items()}
    assert attention_of_state_dict(plain) == 0
    assert attention_of_state_dict({"module." + k: v for k, v in plain.items()}) == 0
    assert attention_of_state_dict(on) == 4 and attention_of_state_dict(wrapped) == 4
    assert attention_of_state_dict(_seeded(dict(OPT, attention="ca", ca_reduction=16)).state_dict()) == 16     # R = 1
    with pytest.raises(ValueError, match="squeeze"):
        attention_of_state_dict({"body.0.ca.squeeze.weight": torch.zeros(3, 16, 1, 1)})
    T = _entry("test")
    for name, sd, want in (("plain", plain, 0), ("on", on, 4), ("wrapped", wrapped, 4)):
        path = str(tmp_path / (name + ".pt"))
        torch.save(sd, path)
        G = T.load_generator(dict(OPT), path, 4)
        found = [m.reduction for m in G.modules() if isinstance(m, ChannelAttention)]
        assert found == [want] * (2 if want else 0), name
        assert T.has_attention(G) == bool(want)
        ref = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        got = G.state_dict()
        assert sorted(got) == sorted(ref) and all(torch.equal(got[k], ref[k]) for k in ref)


def test_pretrained_model_with_other_attention_names_both_flags():
    T = _entry("train")
    on = _seeded(dict(OPT, attention="ca", ca_reduction=4)).state_dict()
    plain = _seeded(OPT).state_dict()
    base = ["--num_channels", "16", "--num_blocks", "2"]
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_attention(on, T.build_parser().parse_args(base), "g.pt")
    assert "--pretrained_model" in str(e.value) and "--attention" in str(e.value) and "--ca_reduction 4" in str(e.value)
    with pytest.raises(SystemExit) as e:
        T.check_pretrained_attention(plain, T.build_parser().parse_args(base + ["--attention", "ca", "--ca_reduction", "4"]), "g.pt")
    assert "--pretrained_model" in str(e.value) and "--attention none" in str(e.value)
    with pytest.raises(SystemExit, match="--ca_reduction 8"):
        T.check_pretrained_attention(on, T.build_parser().parse_args(base + ["--attention", "ca", "--ca_reduction", "8"]), "g.pt")
    assert T.check_pretrained_attention(plain, T.build_parser().parse_args(base), "g.pt") is plain
    assert T.check_pretrained_attention(on, T.build_parser().parse_args(base + ["--attention", "ca", "--ca_reduction", "4"]), "g.pt") is on


def test_state_file_flags():
    from pesr_amd import checkpoint
    T = _entry("train")
    args = lambda *a: T.build_parser().parse_args(["--num_channels", "16", "--num_blocks", "2", *a])
    assert "attention" in checkpoint.SHAPE_FLAGS and checkpoint.FORMAT == 1
    assert checkpoint.shape_flags(args())["attention"] == 0
    assert checkpoint.shape_flags(args("--attention", "ca", "--ca_reduction", "4"))["attention"] == 4
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(args("--attention", "ca", "--ca_reduction", "4"))}
    checkpoint.check_flags(saved, args("--attention", "ca", "--ca_reduction", "4"))
    with pytest.raises(SystemExit, match="--attention"):
        checkpoint.check_flags(saved, args())
    with pytest.raises(SystemExit, match="--attention"):
        checkpoint.check_flags(saved, args("--attention", "ca", "--ca_reduction", "8"))
    # a state written before the flag existed: no such key, counts as none
    old = {"format": checkpoint.FORMAT, "flags": {k: v for k, v in checkpoint.shape_flags(args()).items() if k != "attention"}}
    checkpoint.check_flags(old, args())
    with pytest.raises(SystemExit, match="--attention"):
        checkpoint.check_flags(old, args("--attention", "ca", "--ca_reduction", "4"))


def test_tiling_line_claims_no_exact_halo_with_attention():
    from pesr_amd import tile
    exact = tile.receptive_halo(32, 4)
    plain = tile.describe(32, exact, exact)
    assert "equals" in plain and "APPROXIMATION" not in plain          # (today's line, unchanged)
    assert plain == tile.describe(32, exact, exact, attention=False)
    for halo in (8, exact, exact + 10):
        line = tile.describe(32, halo, exact, attention=True)
        assert "equals" not in line and "APPROXIMATION" in line and "attention" in line


def test_abi_has_the_new_symbols_and_keeps_its_version():
    from pesr_amd import _lib
    names = ["pesr_ca_pool_partials", "pesr_ca_workspace_bytes", "pesr_ca_pool", "pesr_ca_ds", "pesr_ca_gate_fwd", "pesr_ca_apply_fwd",
             "pesr_ca_gate_bwd", "pesr_ca_apply_bwd"]
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert _lib.SIGNATURES[n][1][-1] is _lib._P or n in ("pesr_ca_pool_partials", "pesr_ca_workspace_bytes")      # the stream comes last
    lib = _lib.lib()
    assert lib.pesr_abi_version() == 20
    # the C entry points refuse what Python refuses, with the library's error code and nothing launched (no device here)
    assert lib.pesr_ca_pool_partials(2, 35, 18) == 0 and lib.pesr_ca_workspace_bytes(2, 35, 18, 1) == 0
    assert lib.pesr_ca_pool(None, None, 2, 35, 18, None, 0, None) == -1
    assert lib.pesr_ca_gate_fwd(None, None, None, None, None, None, None, 2, 16, 0, None) == -1
    assert lib.pesr_ca_apply_fwd(None, None, None, None, 2, 35, 18, 0.1, None) == -1


def test_no_cpu_fallback():
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.ca_pool(torch.zeros(1, 4, 4, 16))
