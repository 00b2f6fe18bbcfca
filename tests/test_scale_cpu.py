"""CPU: the x2 / x3 extension of --scale (docs/modes.md section 4e) - model schema and seeded construction, the Discriminator's
classifier width, scale_of_state_dict, train.py's limits, test.py's checkpoint check, the datasets, the ops' CPU refusal."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from scale_oracle import generator_shapes_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("entry_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _opt(C=16, depth=2, scale=None):
    opt = {"num_channels": C, "depth": depth, "res_scale": 0.1}
    if scale is not None:
        opt["scale"] = scale
    return opt


def _plain_torch_generator_sd(C, depth, scale, seed):
    """The Generator's construction restated with plain nn.Conv2d in the same order: trunk, sub_mean, embed, upsampler convs in
    module order, add_mean.  -> state_dict (MeanShift entries excluded: they are overwritten with fixed values)."""
    torch.manual_seed(seed)
    sd = {}
    trunk = []
    for i in range(depth):
        trunk.append((f"body.{i}.body.0", nn.Conv2d(C, C, 3, padding=1)))
        trunk.append((f"body.{i}.body.2", nn.Conv2d(C, C, 3, padding=1)))
    trunk.append((f"body.{depth}", nn.Conv2d(C, C, 3, padding=1)))
    nn.Conv2d(3, 3, 1)                                   # sub_mean's discarded init
    mods = trunk + [("embed", nn.Conv2d(3, C, 3, padding=1))]
    if scale == 4:
        ups = [("upsample.0", 4 * C), ("upsample.2", 4 * C), ("upsample.4", 3)]
    else:
        ups = [("upsample.0", scale * scale * C), ("upsample.2", 3)]
    for name, cout in ups:
        mods.append((name, nn.Conv2d(C, cout, 3, padding=1)))
    for name, m in mods:
        sd[name + ".weight"], sd[name + ".bias"] = m.weight.data, m.bias.data
    return sd


@pytest.mark.parametrize("scale", [2, 3])
def test_state_dict_keys_shapes_and_order(scale):
    from pesr_amd.model import Generator
    G = Generator(_opt(16, 2, scale))
    sd = G.state_dict()
    want = generator_shapes_scaled(16, 2, scale)
    assert list(sd.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(want)
    r = scale
    assert tuple(sd["upsample.0.weight"].shape) == (r * r * 16, 16, 3, 3) and tuple(sd["upsample.2.weight"].shape) == (3, 16, 3, 3)
    assert "upsample.4.weight" not in sd
    assert [type(m).__name__ for m in G.upsample] == ["Conv", "PixelShuffle", "Conv"]
    assert G.upsample[1].upscale_factor == r
    assert G.upsample[0].packed.ps == (scale == 2)


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_seeded_construction_equals_plain_torch(scale):
    from pesr_amd.model import Generator
    want = _plain_torch_generator_sd(16, 2, scale, 7)
    torch.manual_seed(7)
    sd = Generator(_opt(16, 2, scale)).state_dict()
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    assert set(sd) - set(want) == {"sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias"}


def test_default_scale_is_todays_x4():
    from pesr_amd.model import Generator
    from oracle import model as OM
    sds = []
    for scale in (None, 4):
        torch.manual_seed(11)
        sds.append(Generator(_opt(16, 2, scale)).state_dict())
    assert list(sds[0].keys()) == list(sds[1].keys()) == list(OM.generator_shapes(16, 2).keys())
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k
    G = Generator(_opt(16, 2))
    assert [type(m).__name__ for m in G.upsample] == ["Conv", "PixelShuffle", "Conv", "PixelShuffle", "Conv"]
    assert G.upsample[0].packed.ps and G.upsample[2].packed.ps and not G.upsample[4].packed.ps


def test_unsupported_scales_raise():
    from pesr_amd.model import Generator, PixelShuffle, Upsampler
    for bad in (1, 5, 8):
        with pytest.raises(ValueError, match="scale"):
            Generator(_opt(16, 1, bad))
        with pytest.raises(ValueError):
            Upsampler(16, bad)
    with pytest.raises(ValueError):
        PixelShuffle(4)
    assert PixelShuffle(3).upscale_factor == 3


@pytest.mark.parametrize("ps,scale,width", [(48, 2, 512 * 6 * 6), (48, 3, 512 * 9 * 9), (16, 3, 512 * 3 * 3), (48, 4, 512 * 12 * 12)])
def test_discriminator_classifier_width(ps, scale, width):
    from pesr_amd.model import Discriminator
    D = Discriminator({"patch_size": ps, "spectral_norm": False, "scale": scale})
    assert tuple(D.classifier[0].weight.shape) == (1024, width)
    if scale == 4:
        assert tuple(Discriminator({"patch_size": ps, "spectral_norm": False}).classifier[0].weight.shape) == (1024, width)


def test_scale_of_state_dict():
    import model as M          # the drop-in package re-exports it
    from pesr_amd.model import Generator, scale_of_state_dict
    assert M.scale_of_state_dict is scale_of_state_dict
    for scale in (2, 3, 4):
        sd = Generator(_opt(16, 1, scale)).state_dict()
        assert scale_of_state_dict(sd) == scale
        assert scale_of_state_dict({"module." + k: v for k, v in sd.items()}) == scale
    with pytest.raises(ValueError):
        scale_of_state_dict({"embed.weight": torch.zeros(16, 3, 3, 3)})
    with pytest.raises(ValueError):
        scale_of_state_dict({"upsample.0.weight": torch.zeros(48, 16, 3, 3), "upsample.2.weight": torch.zeros(3, 16, 3, 3)})


def test_train_check_limits():
    Tm = _load("train")

    def check(*argv):
        Tm.check_limits(Tm.build_parser().parse_args(list(argv)), 1)

    check("--scale", "2", "--patch_size", "24")                                  # HR 48
    check("--scale", "3", "--patch_size", "16")                                  # HR 48
    check("--scale", "3", "--patch_size", "48")                                  # HR 144
    check("--scale", "2", "--patch_size", "12", "--phase", "pretrain")           # no D / VGG in the pretrain phase
    check("--scale", "3", "--patch_size", "13", "--phase", "pretrain")
    check("--scale", "4", "--patch_size", "24", "--precision", "bf16")
    check("--scale", "3", "--patch_size", "16", "--GP", "true", "--gan_type", "SGAN")
    for bad in ("1", "5", "8"):
        with pytest.raises(SystemExit, match=f"--scale {bad} is not supported"):
            check("--scale", bad)
    with pytest.raises(SystemExit, match=r"\(--patch_size \* --scale\) % 16 == 0, here 12 \* 3 = 36"):
        check("--scale", "3", "--patch_size", "12")
    with pytest.raises(SystemExit, match=r"\(--patch_size \* --scale\) % 16 == 0, here 12 \* 2 = 24"):
        check("--scale", "2", "--patch_size", "12")
    with pytest.raises(SystemExit, match=r"needs --patch_size % 4 == 0"):           # x4 keeps today's wording
        check("--scale", "4", "--patch_size", "22")
    for prec in ("bf16", "split-bf16"):
        with pytest.raises(SystemExit, match=f"--precision {prec} is checked for --scale 4 only"):
            check("--scale", "3", "--patch_size", "16", "--precision", prec)
        with pytest.raises(SystemExit, match="--scale 4 only"):
            check("--scale", "2", "--patch_size", "24", "--precision", prec, "--phase", "pretrain")


def test_test_py_refuses_a_checkpoint_of_another_scale(tmp_path):
    from pesr_amd.model import Generator
    T = _load("test")
    sd3 = Generator(_opt(16, 1, 3)).state_dict()
    assert T.check_checkpoint_scale(sd3, 3, "g3.pt") is sd3
    with pytest.raises(SystemExit, match=r"g3\.pt is a x3 generator, but --scale is 4"):
        T.check_checkpoint_scale(sd3, 4, "g3.pt")
    sd4 = Generator(_opt(16, 1)).state_dict()
    torch.save(sd4, tmp_path / "g4.pt")
    with pytest.raises(SystemExit, match="x4 generator, but --scale is 2"):
        T.load_generator(_opt(16, 1), str(tmp_path / "g4.pt"), 2)
    G = T.load_generator(_opt(16, 1), str(tmp_path / "g4.pt"), 4)
    assert all(torch.equal(G.state_dict()[k], v) for k, v in sd4.items())
    args = T.build_parser().parse_args([])
    assert args.scale == 4
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--scale", "5"])
    with pytest.raises(SystemExit, match="--scale 4 only"):
        T.main(["--scale", "3", "--precision", "bf16"])


@pytest.mark.parametrize("scale", [2, 3])
def test_datasets_at_scale(scale, tmp_path):
    import random
    from PIL import Image
    D = _load("data")
    lr, hr = D.SyntheticSRDataset(2, 8, scale=scale)[1]
    assert lr.shape == (3, 8, 8) and hr.shape == (3, 8 * scale, 8 * scale)
    # the default keeps today's draws: scale 4 and no scale give the same tensors
    a, b = D.SyntheticSRDataset(2, 6)[0], D.SyntheticSRDataset(2, 6, scale=4)[0]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape == (3, 24, 24)
    # a folder whose HR is the nearest-neighbour enlargement of LR: every aligned crop pair then satisfies hr = repeat(lr)
    for sub in ("LR", "HR"):
        (tmp_path / sub).mkdir()
    rng = np.random.RandomState(scale)
    for name, (h, w) in (("a.png", (10, 13)), ("b.png", (9, 9))):
        im = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(im).save(tmp_path / "LR" / name)
        Image.fromarray(im.repeat(scale, 0).repeat(scale, 1)).save(tmp_path / "HR" / name)
    ds = D.FolderSRDataset(str(tmp_path), 5, num_repeats=3, is_aug=True, scale=scale)
    random.seed(0)
    for i in range(len(ds)):
        l, h = ds[i]
        assert l.shape == (3, 5, 5) and h.shape == (3, 5 * scale, 5 * scale)
        assert torch.equal(h, l.repeat_interleave(scale, 1).repeat_interleave(scale, 2))
    full = D.FolderSRDataset(str(tmp_path), None, scale=scale)
    l, h = full[0]
    assert h.shape == (3, 10 * scale, 13 * scale)
    # an HR of the wrong size fails with the file name
    Image.fromarray(rng.randint(0, 256, (9 * 4, 9 * 4, 3)).astype(np.uint8)).save(tmp_path / "HR" / "b.png")
    with pytest.raises(ValueError, match=r"b\.png.*scale " + str(scale)):
        full[1]


def test_new_ops_have_no_cpu_fallback():
    from pesr_amd import _lib, ops
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.pixel_shuffle_r_fwd(torch.zeros(1, 2, 2, 9), 3)
    with pytest.raises(_lib.PesrHipError, match="no CPU fallback"):
        ops.pixel_shuffle_r_bwd(torch.zeros(1, 6, 6, 1), 3)
