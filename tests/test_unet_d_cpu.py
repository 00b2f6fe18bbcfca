"""CPU: the pieces of the U-Net discriminator (--d_arch unet, docs/modes.md section 4v) that need no GPU - the flags and their refusals,
seeded construction with and without spectral norm, the unchanged default, the state file's flag and the C ABI."""
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry(name):
    spec = importlib.util.spec_from_file_location("entry_unet_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_train_flags_exist_with_defaults():
    p = _entry("train").build_parser()
    a = p.parse_args([])
    assert a.d_arch == "vgg" and a.d_width == 64
    a = p.parse_args(["--d_arch", "unet", "--d_width", "32"])
    assert a.d_arch == "unet" and a.d_width == 32
    with pytest.raises(SystemExit):
        p.parse_args(["--d_arch", "patch"])


@pytest.mark.parametrize("argv, what", [
    (["--d_arch", "unet", "--d_width", "24", "--phase", "train"], ["--d_width"]),
    (["--d_width", "0", "--phase", "train"], ["--d_width"]),
    (["--d_width", "-16", "--phase", "pretrain"], ["--d_width"]),
    (["--GP", "true", "--d_arch", "unet", "--phase", "train"], ["--GP", "--d_arch"]),
    (["--d_arch", "unet", "--phase", "train", "--scale", "2", "--patch_size", "10"], ["--d_arch", "--patch_size"]),
])
def test_train_refuses_before_any_device(argv, what, monkeypatch):
    T = _entry("train")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        T.main(argv + ["--synthetic", "4"])
    for w in what:
        assert w in str(e.value), str(e.value)


def test_pretrain_accepts_the_flag_and_does_not_use_it():
    T = _entry("train")
    assert T.d_arch_of(T.build_parser().parse_args(["--phase", "pretrain", "--d_arch", "unet", "--GP", "true"])) == "unet"
    from pesr_amd import checkpoint
    flags = checkpoint.shape_flags(T.build_parser().parse_args(["--phase", "pretrain", "--d_arch", "unet"]))
    assert flags["d_arch"] == "vgg"           # the pretrain phase has no Discriminator: its state says nothing about one


def _seeded(opt, seed=0):
    from pesr_amd.model import UNetDiscriminator
    torch.manual_seed(seed)
    return UNetDiscriminator(opt)


PLAN = [(3, 1, 1, True), (1, 2, 2, False), (2, 4, 2, False), (4, 8, 2, False), (8, 4, 1, False), (4, 2, 1, False), (2, 1, 1, False),
        (1, 1, 1, False), (1, 1, 1, False), (1, None, 1, True)]     # (cin / w, cout / w, stride, bias); conv0's cin is 3, conv9's cout 1


@pytest.mark.parametrize("sn", [False, True])
@pytest.mark.parametrize("w", [64, 16])
def test_seeded_construction_keys_shapes_count_and_rng_order(sn, w):
    D = _seeded({"spectral_norm": sn, "d_width": w} if w != 64 else {"spectral_norm": sn})
    sd = D.state_dict()
    want, count = {}, 0
    torch.manual_seed(0)
    for i, (ci, co, stride, bias) in enumerate(PLAN):
        cin, cout = (3 if i == 0 else ci * w), (1 if co is None else co * w)
        ref = torch.nn.Conv2d(cin, cout, 3, padding=1, stride=stride, bias=bias)
        has_sn = sn and 1 <= i <= 8
        want[f"conv{i}.weight_orig" if has_sn else f"conv{i}.weight"] = ref.weight.data
        count += ref.weight.numel()
        if bias:
            want[f"conv{i}.bias"] = ref.bias.data
            count += cout
        if has_sn:          # u, then v, right after the conv they belong to (torch.nn.utils.spectral_norm's draws)
            want[f"conv{i}.weight_u"] = torch.nn.functional.normalize(torch.empty(cout).normal_(0, 1), dim=0, eps=1e-12)
            want[f"conv{i}.weight_v"] = torch.nn.functional.normalize(torch.empty(cin * 9).normal_(0, 1), dim=0, eps=1e-12)
        assert D.get_submodule(f"conv{i}").stride == stride
    assert sorted(sd) == sorted(want)
    for k in want:
        assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]), k
    assert sum(p.numel() for p in D.parameters()) == count
    if w == 64:
        assert count == 3_172_673         # about 3.2 M parameters, against the VGG-style D's 80 M


def test_patch_size_does_not_matter_and_bad_widths_raise():
    a = _seeded({"spectral_norm": False, "patch_size": 24}).state_dict()
    b = _seeded({"spectral_norm": False, "patch_size": 48, "scale": 2}).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="d_width"):
        _seeded({"spectral_norm": False, "d_width": 6})
    with pytest.raises(ValueError, match="d_width"):
        _seeded({"spectral_norm": False, "d_width": 0})


def test_it_is_no_discriminator_for_the_pairing_path():
    from pesr_amd.model import Discriminator
    D = _seeded({"spectral_norm": False, "d_width": 16})
    assert not isinstance(D, Discriminator) and not hasattr(D, "forward_second_order")
    with pytest.raises(TypeError, match="classifier"):
        D.forward_features(torch.zeros(1, 3, 8, 8))
    with pytest.raises(TypeError, match="classifier"):
        D.classify_pair(None, None)


@pytest.mark.parametrize("shape", [(1, 3, 12, 16), (1, 3, 16, 12), (1, 3, 4, 8), (1, 1, 8, 8), (3, 8, 8)])
def test_forward_refuses_a_size_naming_it(shape):
    D = _seeded({"spectral_norm": False, "d_width": 16})
    with pytest.raises(ValueError, match=re.escape(str(tuple(shape)))):
        D(torch.zeros(shape))


def test_trainer_refuses_the_gradient_penalty():
    from pesr_amd.step import Trainer
    D = _seeded({"spectral_norm": False, "d_width": 16})
    with pytest.raises(ValueError, match="gradient_penalty"):
        Trainer(None, D, gradient_penalty=True)
    Trainer(None, D)


def test_default_flags_still_build_todays_discriminator():
    from helpers import dis_sd
    from pesr_amd.model import Discriminator
    T = _entry("train")
    assert T.d_arch_of(T.build_parser().parse_args([])) == "vgg"
    opt = {"patch_size": 8, "spectral_norm": False}
    torch.manual_seed(0)
    a = Discriminator(opt).state_dict()
    torch.manual_seed(0)
    b = Discriminator(dict(opt, d_width=64)).state_dict()        # (the key the new class reads means nothing to this one)
    assert list(a) == list(b) and sorted(a) == sorted(dis_sd(8)) and all(torch.equal(a[k], b[k]) for k in a)
    # today's seeded values: the stem is nn.Conv2d's first draw after the seed
    torch.manual_seed(0)
    ref = torch.nn.Conv2d(3, 64, 3, padding=1, bias=False)
    assert torch.equal(a["features.0.0.weight"], ref.weight.data)


def test_state_file_flag():
    from pesr_amd import checkpoint
    T = _entry("train")
    args = lambda *a: T.build_parser().parse_args(["--phase", "train", "--num_channels", "16", "--num_blocks", "2", *a])
    assert "d_arch" in checkpoint.SHAPE_FLAGS and checkpoint.FORMAT == 1
    assert checkpoint.shape_flags(args())["d_arch"] == "vgg"
    assert checkpoint.shape_flags(args("--d_arch", "unet"))["d_arch"] == "unet"
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(args("--d_arch", "unet"))}
    checkpoint.check_flags(saved, args("--d_arch", "unet"))
    with pytest.raises(SystemExit, match="--d_arch"):
        checkpoint.check_flags(saved, args())
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(args())}
    with pytest.raises(SystemExit, match="--d_arch"):
        checkpoint.check_flags(saved, args("--d_arch", "unet"))
    # a state written before the flag existed: no such key, counts as vgg
    old = {"format": checkpoint.FORMAT, "flags": {k: v for k, v in checkpoint.shape_flags(args()).items() if k != "d_arch"}}
    checkpoint.check_flags(old, args())
    with pytest.raises(SystemExit, match="--d_arch"):
        checkpoint.check_flags(old, args("--d_arch", "unet"))


NEW_SYMBOLS = ["pesr_bilinear_up2_fwd", "pesr_bilinear_up2_bwd", "pesr_gan_loss_map_workspace_bytes", "pesr_gan_loss_map",
               "pesr_conv3x3_c1_wgrad_workspace_bytes", "pesr_conv3x3_c1_fwd", "pesr_conv3x3_c1_dgrad", "pesr_conv3x3_c1_wgrad"]


def test_abi_has_the_new_symbols_and_keeps_its_version():
    from pesr_amd import _lib
    header = open(os.path.join(ROOT, "include", "pesr_hip.h")).read()
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n                                     # exported
        assert _lib.SIGNATURES[n][1][-1] is _lib._P or n.endswith("_workspace_bytes")      # the stream comes last
    assert lib.pesr_abi_version() == 20
    # bad arguments: the library's error code with nothing launched (no device here)
    assert lib.pesr_bilinear_up2_fwd(None, None, None, 1, 4, 4, 4, None) == -1
    assert lib.pesr_bilinear_up2_bwd(None, None, 1, 0, 4, 4, None) == -1
    assert lib.pesr_gan_loss_map_workspace_bytes(0) == 0 and lib.pesr_gan_loss_map_workspace_bytes(1) == 64 + 20
    assert lib.pesr_gan_loss_map_workspace_bytes(70000) == 64 + 69 * 20          # 69 rows of 1024 logits, the last one ragged
    assert lib.pesr_gan_loss_map(None, None, 0, 0, 0, 0, 1.0, 1.0, None, None, None, None, 0, None) == -1
    assert lib.pesr_conv3x3_c1_wgrad_workspace_bytes(2, 8, 8, 18) == 0 and lib.pesr_conv3x3_c1_wgrad_workspace_bytes(2, 8, 8, 64) > 0
    assert lib.pesr_conv3x3_c1_fwd(None, None, None, None, 2, 8, 8, 18, None) == -1
    assert lib.pesr_conv3x3_c1_dgrad(None, None, None, 2, 8, 8, 2048, None) == -1
    assert lib.pesr_conv3x3_c1_wgrad(None, None, None, None, 2, 8, 8, 64, 1.0, None, 0, None) == -1


def test_the_routed_3x3_path_takes_no_one_channel_gradient():
    """Why conv9 has kernels of its own: the implicit-GEMM entry points refuse Cout = 1 on the input-gradient and weight-gradient side."""
    from pesr_amd import _lib, ops
    lib = _lib.lib()
    assert lib.pesr_conv3x3_wgrad_workspace_bytes(2, 16, 16, 64, 1, 1, 0) == 0
    assert lib.pesr_conv3x3_dgrad(None, None, None, None, None, 2, 16, 16, 64, 1, 1, 1.0, 0, None, 0, None) == -1
    assert ops.c1_eligible(64, 1, 1) and not ops.c1_eligible(64, 1, 2) and not ops.c1_eligible(64, 3, 1) and not ops.c1_eligible(6, 1, 1)


def test_no_cpu_fallback_and_refusals_name_the_argument():
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.bilinear_up2_fwd(torch.zeros(1, 4, 4, 16))
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.gan_loss_map(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4), "SGAN", 0, False, 1.0)
