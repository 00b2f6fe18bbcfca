"""CPU: the pieces of resumable training that need no GPU - train.py's new flags, FlatAdam's state in torch.optim.Adam's schema,
the state file's flag check, its atomic write and --resume's path resolution (pesr_amd/checkpoint.py, docs/modes.md section 4i)."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMELS = (1, 5, 8)       # flat offsets 0, 4, 12 and 20 floats in all: the first two parameters are followed by padding


def _train():
    spec = importlib.util.spec_from_file_location("entry_train", os.path.join(ROOT, "train.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(1,), (5,), (2, 4)]
    assert tuple(torch.Size(s).numel() for s in shapes) == NUMELS
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _filled(ema_decay=0.0, seed=0, steps=7):
    from pesr_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(100 + seed)
    opt = FlatAdam(_params(seed), lr=3e-4, betas=(0.8, 0.95), eps=1e-7, ema_decay=ema_decay)
    opt.exp_avg.copy_(torch.randn(opt.flat.numel, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.flat.numel, generator=g))
    if opt.flat_ema is not None:
        opt.flat_ema.copy_(torch.randn(opt.flat.numel, generator=g))
    opt.steps = steps
    return opt


def test_flag_defaults_reproduce_todays_run():
    a = _train().build_parser().parse_args([])
    assert a.save_state_every == 0 and a.resume == "" and a.ema_decay == 0.0
    a = _train().build_parser().parse_args(["--resume", "auto", "--save_state_every", "5", "--ema_decay", "0.999"])
    assert a.resume == "auto" and a.save_state_every == 5 and a.ema_decay == 0.999


def test_state_dict_loads_into_torch_adam_and_comes_back_bit_equal():
    from pesr_amd.optim import FlatAdam
    opt = _filled()
    assert opt.flat.offsets == [0, 4, 12] and opt.flat.numel == 20
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1, 2]
    g = sd["param_groups"][0]
    assert g["lr"] == 3e-4 and tuple(g["betas"]) == (0.8, 0.95) and g["eps"] == 1e-7 and g["params"] == [0, 1, 2]
    for i, p in enumerate(opt.flat.params):
        st = sd["state"][i]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) == 7
        o = opt.flat.offsets[i]
        assert torch.equal(st["exp_avg"].reshape(-1), opt.exp_avg[o:o + p.numel()])
    # torch.optim.Adam over the same parameter list takes it, keeps the values, and can step with it
    ref = torch.optim.Adam(opt.flat.params, lr=1.0)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["lr"] == 3e-4 and tuple(ref.param_groups[0]["betas"]) == (0.8, 0.95)
    for i, p in enumerate(opt.flat.params):
        assert torch.equal(ref.state[p]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(ref.state[p]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert float(ref.state[p]["step"]) == 7
    back = ref.state_dict()
    # ... and the reverse: torch.optim.Adam's own state_dict into a differently filled FlatAdam
    other = _filled(seed=1, steps=2)
    other.exp_avg.fill_(9.0); other.exp_avg_sq.fill_(9.0)        # (the padding too)
    other.load_state_dict(back)
    assert other.steps == 7 and other.param_groups[0]["lr"] == 3e-4 and tuple(other.param_groups[0]["betas"]) == (0.8, 0.95)
    sd2 = other.state_dict()
    for i in range(3):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][i][k], sd["state"][i][k]), (i, k)
        assert float(sd2["state"][i]["step"]) == 7
    for p in opt.flat.params:
        p.grad = torch.ones_like(p)
    ref.step()                                                    # (no option of torch.optim.Adam is missing from the groups)
    fresh = FlatAdam(_params(3))
    assert fresh.state_dict()["state"] == {}                      # like torch.optim.Adam before its first step
    other.load_state_dict(fresh.state_dict())
    assert other.steps == 0 and other.state_dict()["state"] == {}
    for p, o in zip(other.flat.params, other.flat.offsets):      # an empty state means zero moments
        assert not other.exp_avg[o:o + p.numel()].any() and not other.exp_avg_sq[o:o + p.numel()].any()


def test_alignment_padding_never_leaks():
    """Numels 1, 5, 8: the flat buffers hold 3 + 3 floats of padding.  Poisoned padding is not in the state, and a load leaves the
    receiving optimizer's padding alone."""
    opt = _filled(ema_decay=0.9)
    pad = torch.ones(20, dtype=torch.bool)
    for p, o in zip(opt.flat.params, opt.flat.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) == 6
    for flat in (opt.exp_avg, opt.exp_avg_sq, opt.flat_ema):
        flat[pad] = float("nan")
    sd = opt.state_dict()
    tensors = [t for st in sd["state"].values() for t in (st["exp_avg"], st["exp_avg_sq"])] + list(sd["ema"])
    assert [t.numel() for t in sd["ema"]] == list(NUMELS) and sum(t.numel() for t in tensors) == 3 * 14
    assert all(bool(torch.isfinite(t).all()) for t in tensors)
    assert sd["ema_decay"] == 0.9
    other = _filled(ema_decay=0.9, seed=1)
    for flat in (other.exp_avg, other.exp_avg_sq, other.flat_ema):
        flat[pad] = 123.0
    other.load_state_dict(sd)
    for a, b in ((other.exp_avg, opt.exp_avg), (other.exp_avg_sq, opt.exp_avg_sq), (other.flat_ema, opt.flat_ema)):
        assert torch.equal(a[~pad], b[~pad]) and bool((a[pad] == 123.0).all())


def test_shape_and_ema_mismatch_messages():
    opt = _filled()
    sd = opt.state_dict()
    sd["state"][1]["exp_avg_sq"] = torch.zeros(2, 3)
    before = opt.exp_avg.clone()
    with pytest.raises(ValueError, match=r"parameter 1: exp_avg_sq has shape \(2, 3\) in the state, the parameter has \(5,\)"):
        opt.load_state_dict(sd)
    assert torch.equal(opt.exp_avg, before) and opt.steps == 7          # refused before anything was written
    with pytest.raises(ValueError, match="without a moving average"):
        _filled(ema_decay=0.5).load_state_dict(_filled().state_dict())
    with pytest.raises(ValueError, match="with a moving average"):
        _filled().load_state_dict(_filled(ema_decay=0.5).state_dict())
    sd = _filled().state_dict()
    sd["param_groups"][0]["params"] = [0, 1]
    with pytest.raises(ValueError, match="2 parameters"):
        _filled().load_state_dict(sd)
    from pesr_amd.optim import FlatAdam
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdam(_params(), ema_decay=1.0)
    with pytest.raises(ValueError, match="no moving average"):
        _filled().ema_module(torch.nn.Linear(2, 2))


def _args(**kw):
    a = _train().build_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_state_file_flag_mismatch_names_the_flag_and_both_values():
    from pesr_amd import checkpoint
    saved = {"format": checkpoint.FORMAT, "flags": checkpoint.shape_flags(_args(num_channels=64, num_blocks=2, ema_decay=0.9))}
    checkpoint.check_flags(saved, _args(num_channels=64, num_blocks=2, ema_decay=0.999))      # another decay is no mismatch
    with pytest.raises(SystemExit, match=r"--num_blocks = 2, this run has 32"):
        checkpoint.check_flags(saved, _args(num_channels=64, ema_decay=0.9))
    with pytest.raises(SystemExit, match=r"--phase = 'train', this run has 'pretrain'"):
        checkpoint.check_flags(saved, _args(num_channels=64, num_blocks=2, ema_decay=0.9, phase="pretrain"))
    with pytest.raises(SystemExit, match=r"--scale = 4, this run has 2"):
        checkpoint.check_flags(saved, _args(num_channels=64, num_blocks=2, ema_decay=0.9, scale=2))
    with pytest.raises(SystemExit, match=r"--spectral_norm = False, this run has True"):
        checkpoint.check_flags(saved, _args(num_channels=64, num_blocks=2, ema_decay=0.9, spectral_norm=True))
    with pytest.raises(SystemExit, match=r"--ema_decay > 0 = True, this run has False"):
        checkpoint.check_flags(saved, _args(num_channels=64, num_blocks=2))
    with pytest.raises(SystemExit, match="format 99"):
        checkpoint.check_flags({**saved, "format": 99}, _args(num_channels=64, num_blocks=2, ema_decay=0.9))


def test_atomic_write_keeps_the_old_file_when_the_save_dies(tmp_path, monkeypatch):
    from pesr_amd import checkpoint
    path = str(tmp_path / "train_state.pt")
    checkpoint.atomic_save({"epoch": 1, "w": torch.arange(4.0)}, path)
    assert not os.path.exists(path + ".tmp")
    real = torch.save

    def dies_midway(obj, f, *a, **kw):
        real(obj, f, *a, **kw)
        with open(f, "r+b") as fh:       # half a file is on the disk when the process is hit
            fh.truncate(os.path.getsize(f) // 2)
        raise KeyboardInterrupt

    monkeypatch.setattr(torch, "save", dies_midway)
    with pytest.raises(KeyboardInterrupt):
        checkpoint.atomic_save({"epoch": 2, "w": torch.zeros(4)}, path)
    monkeypatch.setattr(torch, "save", real)
    old = checkpoint.load_state(path)
    assert old["epoch"] == 1 and torch.equal(old["w"], torch.arange(4.0))
    assert os.listdir(tmp_path) == ["train_state.pt"]
    checkpoint.atomic_save({"epoch": 3, "w": torch.ones(4)}, path)
    assert checkpoint.load_state(path)["epoch"] == 3


def test_resume_path_resolution(tmp_path):
    from pesr_amd import checkpoint
    ck = str(tmp_path / "ck")
    assert checkpoint.resolve_resume("", ck, "train") is None
    assert checkpoint.resolve_resume("auto", ck, "train") is None                       # nothing there yet: a fresh start
    own = checkpoint.state_path(ck, "train")
    assert own == os.path.join(ck, "train", "train_state.pt")
    os.makedirs(os.path.dirname(own))
    checkpoint.atomic_save({"epoch": 1}, own)
    assert checkpoint.resolve_resume("auto", ck, "train") == own
    assert checkpoint.resolve_resume("auto", ck, "pretrain") is None                    # the other phase has its own file
    assert checkpoint.resolve_resume(own, "elsewhere", "pretrain") == own
    with pytest.raises(SystemExit, match="no such file"):
        checkpoint.resolve_resume(str(tmp_path / "missing.pt"), ck, "train")


def test_rng_snapshot_restores_every_host_stream():
    import random

    import numpy as np
    from pesr_amd import checkpoint

    class Loader:
        rng = random.Random(5)
    snap = checkpoint.rng_snapshot(None, Loader)
    first = (torch.rand(3), random.random(), np.random.rand(), Loader.rng.random())
    checkpoint.rng_restore(snap, None, Loader)
    again = (torch.rand(3), random.random(), np.random.rand(), Loader.rng.random())
    assert torch.equal(first[0], again[0]) and first[1:] == again[1:]
    assert checkpoint.gather_rng(snap, 0, 1) == [snap]
