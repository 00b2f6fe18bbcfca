"""GPU: resumable training (docs/modes.md section 4i) - FlatAdam's state and moving average at Trainer level, ema_module, and
train.py --save_state_every / --resume / --ema_decay end to end: a run stopped at an epoch boundary and resumed leaves the same
bits as the run that was never stopped."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import dis_sd, gen_sd, vgg_sd
from oracle import detrand
from oracle import model as OM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, DEPTH, PS, BATCH, DECAY, LR = 64, 2, 8, 4, 0.9, 5e-5
_SHARED = {}


def _vgg():
    if "vgg" not in _SHARED:        # frozen: one instance serves every trainer of this file
        from model import VGG
        V = VGG(); V.load_state_dict(vgg_sd()); V.cuda()
        _SHARED["vgg"] = V
    return _SHARED["vgg"]


def _data():
    if "data" not in _SHARED:
        _SHARED["data"] = [(detrand.image_batch((BATCH, 3, PS, PS), 150 + i).cuda(),
                            detrand.image_batch((BATCH, 3, 4 * PS, 4 * PS), 160 + i).cuda()) for i in range(6)]
    return _SHARED["data"]


def _trainer(seed, gp=False):
    from model import Discriminator, Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = Generator({"num_channels": C, "depth": DEPTH, "res_scale": 0.1, "scale": 4}); G.load_state_dict(gen_sd(C, DEPTH, seed)); G.cuda()
    D = Discriminator({"patch_size": PS, "spectral_norm": False}); D.load_state_dict(dis_sd(PS, seed + 1)); D.cuda()
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=LR, betas=(0.9, 0.999), ema_decay=DECAY)
    oD = FlatAdam(D.parameters(), lr=LR, betas=(0.9, 0.999))
    return Trainer(G, D, _vgg(), oG, oD, gradient_penalty=gp)


def _snapshot(tr):
    snap = {"D." + k: v.clone() for k, v in tr.D.state_dict().items()}       # (BatchNorm running statistics among them)
    for name, o in (("G", tr.optim_G), ("D", tr.optim_D)):
        snap[name + ".flat_p"], snap[name + ".exp_avg"], snap[name + ".exp_avg_sq"] = o.flat.flat_p.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()
        snap[name + ".steps"] = o.steps
    snap["G.flat_ema"] = tr.optim_G.flat_ema.clone()
    return snap


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs, max {float((a[k].double() - b[k].double()).abs().max()):.3e}"
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _logs(d):
    return {k: v.item() for k, v in d.items()}


def _reference(gp):
    """Six uninterrupted eager steps from seed 0 (computed once per flavour): the state after steps 4 and 6, the losses of 3..6."""
    key = ("ref", gp)
    if key not in _SHARED:
        if gp:
            torch.cuda.manual_seed(4321)
        tr = _trainer(0, gp)
        out = {"logs": []}
        for i, (lr, hr) in enumerate(_data()):
            out["logs"].append(_logs(tr.gan_step(lr, hr)))
            if i + 1 in (4, 6):
                out[i + 1] = _snapshot(tr)
        _SHARED[key] = out
    return _SHARED[key]


def _saved_after_two_steps(tmp_path, gp):
    """Two steps from seed 0, then everything a resumed run needs goes through torch.save to a file and is read back."""
    from pesr_amd import checkpoint
    if gp:
        torch.cuda.manual_seed(4321)
    tr = _trainer(0, gp)
    for lr, hr in _data()[:2]:
        tr.gan_step(lr, hr)
    path = str(tmp_path / "state.pt")
    checkpoint.atomic_save({"G": tr.G.state_dict(), "D": tr.D.state_dict(), "optim_G": tr.optim_G.state_dict(),
                            "optim_D": tr.optim_D.state_dict(), "rng": checkpoint.rng_snapshot("cuda")}, path)
    if gp:
        torch.rand(1000, device="cuda")          # the stream moves on: only a restore brings the same interpolation weights
    return checkpoint.load_state(path)


def _load(tr, st):
    tr.G.load_state_dict(st["G"]); tr.D.load_state_dict(st["D"])
    tr.optim_G.load_state_dict(st["optim_G"]); tr.optim_D.load_state_dict(st["optim_D"])


@pytest.mark.parametrize("mode", ["eager", "device-state", "hipgraph", "gp"])
def test_trainer_state_saved_and_loaded_into_fresh_objects_continues_bit_identically(tmp_path, mode):
    from pesr_amd import checkpoint
    gp = mode == "gp"
    ref = _reference(gp)
    st = _saved_after_two_steps(tmp_path, gp)
    tr = _trainer(40, gp)                        # other weights, zero moments, its own BatchNorm statistics
    assert not torch.equal(tr.optim_G.flat.flat_p, ref[4]["G.flat_p"])
    if mode == "device-state":
        tr.optim_G.use_device_state(); tr.optim_D.use_device_state()      # load_state_dict must rewrite the device count and lr
    _load(tr, st)
    assert tr.optim_G.steps == tr.optim_D.steps == 2
    if gp:
        checkpoint.rng_restore(st["rng"], "cuda")
    data = _data()
    logs = [_logs(tr.gan_step(lr, hr)) for lr, hr in data[2:4]]
    assert logs == ref["logs"][2:4], (logs, ref["logs"][2:4])
    _same(_snapshot(tr), ref[4], mode + " after step 4")
    if mode == "device-state":
        assert tr.optim_G.dev_state.view(torch.int32)[4].item() == 4 and tr.optim_G.dev_state[0].item() == np.float32(LR)
    if mode == "hipgraph":
        step = tr.capture_gan_step(*data[0])     # (two eager steps since the load, as train.py does)
        logs = [_logs(step(lr, hr)) for lr, hr in data[4:6]]
        assert logs == ref["logs"][4:6], (logs, ref["logs"][4:6])
        _same(_snapshot(tr), ref[6], "replays after step 6")


def test_load_state_dict_refuses_a_state_of_other_shapes_on_the_device():
    tr = _trainer(0)
    sd = tr.optim_G.state_dict()
    sd["ema"][3] = torch.zeros(2, 2)
    with pytest.raises(ValueError, match=r"parameter 3: ema has shape \(2, 2\) in the state, the parameter has \("):
        tr.optim_G.load_state_dict(sd)


def test_ema_module_reads_the_averaged_weights():
    from model import Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    opt = {"num_channels": C, "depth": DEPTH, "res_scale": 0.1, "scale": 4}
    G = Generator(opt); G.load_state_dict(gen_sd(C, DEPTH, 5)); G.cuda()
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=1e-3, ema_decay=DECAY)
    tr = Trainer(G, optim_G=oG)
    E = oG.ema_module(G)
    assert type(E) is Generator and E is not G and not E.training
    assert all(not p.requires_grad for p in E.parameters())
    lo, hi = oG.flat_ema.data_ptr(), oG.flat_ema.data_ptr() + 4 * oG.flat_ema.numel()
    assert all(lo <= p.data_ptr() < hi for p in E.parameters())                 # views, not copies
    assert list(E.state_dict().keys()) == list(OM.generator_shapes(C, DEPTH).keys())
    x = detrand.image_batch((1, 3, 10, 14), 77).cuda()
    one_minus_d = float(np.float32(1.0) - np.float32(DECAY))
    e64 = {k: v.double() for k, v in G.state_dict().items()}

    def plain_forward():
        P = Generator(opt); P.load_state_dict({k: v.clone() for k, v in E.state_dict().items()}); P.cuda().eval()
        with torch.no_grad():
            return P(x)

    def steps(n, first):
        for i in range(n):
            lr, hr = _data()[(first + i) % 6]
            tr.pretrain_step(lr, hr)
            for k, v in G.state_dict().items():
                e64[k] = e64[k] + (v.double() - e64[k]) * one_minus_d

    def check_recurrence(k_steps):
        live = G.state_dict()
        for k, v in E.state_dict().items():
            bound = k_steps * 2.0 ** -22 * torch.maximum(v.abs(), live[k].abs()).double()
            assert bool(((v.double() - e64[k]).abs() <= bound).all()), k
        assert any(not torch.equal(v, live[k]) for k, v in E.state_dict().items())

    steps(3, 0)
    check_recurrence(3)
    oG.refresh_ema()
    with torch.no_grad():
        y1 = E(x)
    assert torch.equal(y1, plain_forward())
    with torch.no_grad():
        assert not torch.equal(y1, G(x))                                     # the averaged weights are not the live ones
    steps(2, 3)
    check_recurrence(5)
    oG.refresh_ema()
    with torch.no_grad():
        y2 = E(x)
    assert not torch.equal(y2, y1)                                           # stale packed weights would have served y1 again
    assert torch.equal(y2, plain_forward())


# ---- train.py end to end -----------------------------------------------------------------------------------------------------
PROG = """
import importlib.util, os, shutil, sys
sys.path.insert(0, {root!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({root!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
base = {base!r}
def run(tag, epochs, resume=None, extra=()):
    print("RUN_" + tag, flush=True)
    args = ["--num_channels", "64", "--num_blocks", "2", "--patch_size", "8", "--batch_size", "4", "--max_iters", "4", "--lr_step", "2",
            "--snapshot_every", "1", "--num_epochs", str(epochs), "--check_point", os.path.join(base, tag)] + {common!r} + list(extra)
    if resume is not None:
        copy = os.path.join(base, "from_" + tag + ".pt")
        shutil.copyfile(os.path.join(base, resume, "train", "train_state.pt"), copy)
        args += ["--resume", copy]
    Tm.main(args)
new = ["--save_state_every", "1", "--ema_decay", "0.9"]
run("a", 1, extra=new)
run("b", 3, "a", new)
run("c", 2, "a", new)
run("d", 3, "c", new)
if {plain!r}:
    run("plain", 1)
print("ENTRY_OK")
"""


def _tensors(obj, prefix=""):
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _tensors(v, f"{prefix}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, f"{prefix}/{i}")


@pytest.mark.parametrize("mode", ["eager", "hipgraph", "gpu_pipeline"])
def test_train_py_stopped_and_resumed_equals_the_uninterrupted_run(tmp_path, mode):
    """(a) one epoch -> S1.  (b) resumes S1 and runs epochs 2 and 3; (c) resumes S1 and stops after epoch 2; (d) resumes (c)'s state
    for epoch 3.  (b) and (d) must leave the same model_3.pt and the same train_state.pt, tensor for tensor.  Every run starts from
    S1, so D's unseeded initialisation does not matter; --lr_step 2 halves the rate across the cut (scheduler restore); a lost
    random stream would shuffle (b) and (d) differently.  The eager case also runs today's command line: no state file, no EMA."""
    from pesr_amd import checkpoint
    if mode == "gpu_pipeline":
        from PIL import Image
        rng = np.random.RandomState(8)
        for sub, count in (("train", 6), ("valid", 1)):
            d = tmp_path / "data" / "origin" / sub / "Toy" / "HR"
            d.mkdir(parents=True)
            for i in range(count):
                Image.fromarray(rng.randint(0, 256, (40, 40, 3)).astype(np.uint8)).save(d / f"{i}.png")
        common = ["--train_dataset", "Toy", "--valid_dataset", "Toy", "--num_repeats", "4", "--gpu_pipeline", "true", "--lr_from_hr", "true",
                  "--allow_random_vgg", "true", "--hip_graph", "false"]
    else:
        common = ["--synthetic", "16", "--hip_graph", "true" if mode == "hipgraph" else "false"]
    base = str(tmp_path / "ck")
    prog = PROG.format(root=ROOT, base=base, common=common, plain=mode == "eager")
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {m.group(1): m.group(2) for m in re.finditer(r"RUN_(\w+)\n(.*?)(?=RUN_|ENTRY_OK)", r.stdout, flags=re.S)}
    assert "Finish valid [1/1]. PSNR:" in out["a"] and out["a"].count(" (EMA)") == 1
    assert re.search(r"Epoch \[2/3\] lr 5e-05 ", out["b"]) and re.search(r"Epoch \[3/3\] lr 2.5e-05 ", out["b"]), out["b"][-1500:]
    assert "Epoch [1/" not in out["b"] and "Epoch [2/" not in out["d"] and re.search(r"Epoch \[3/3\] lr 2.5e-05 ", out["d"]), out["d"][-1500:]
    assert re.search(r"^resume: .*epoch 2 done, going on with epoch 3 at lr 2.5e-05", out["d"], flags=re.M), out["d"][-1500:]

    def load(tag, name):
        return torch.load(os.path.join(base, tag, "train", name), map_location="cpu", weights_only=False)
    mb, md = load("b", "model_3.pt"), load("d", "model_3.pt")
    assert list(mb.keys()) == list(OM.generator_shapes(C, DEPTH).keys())          # the reference's checkpoint schema
    for k in mb:
        assert torch.equal(mb[k], md[k]), k
    sb, sd = load("b", "train_state.pt"), load("d", "train_state.pt")
    assert sb["epoch"] == sd["epoch"] == 3 and sb["format"] == checkpoint.FORMAT and sb["flags"] == sd["flags"]
    tb, td = dict(_tensors(sb)), dict(_tensors(sd))
    assert list(tb) == list(td)
    for part in ("/G/", "/D/", "/optim_G/state/", "/optim_G/ema/", "/optim_D/state/", "/rng/0/torch", "/rng/0/device"):
        assert any(k.startswith(part) for k in tb), part
    for k in tb:
        assert torch.equal(tb[k], td[k]), k
    assert sb["scheduler_G"] == sd["scheduler_G"] and sb["scheduler_D"] == sd["scheduler_D"] and sb["scheduler_G"]["last_epoch"] == 3
    assert sb["rng"][0]["python"] == sd["rng"][0]["python"]
    assert ("shuffle" in sb["rng"][0]) == (mode != "gpu_pipeline")          # (a tensor: compared above)
    assert ("gpu_loader" in sb["rng"][0]) == (mode == "gpu_pipeline")
    if mode == "gpu_pipeline":
        assert sb["rng"][0]["gpu_loader"] == sd["rng"][0]["gpu_loader"]
    # the saved model is the average; the raw weights are in the state file; it trained between the epochs
    assert any(not torch.equal(mb[k], sb["G"][k]) for k in mb)
    for k, e in zip([n for n in mb if n in sb["G"]], sb["optim_G"]["ema"]):
        assert torch.equal(mb[k], e), k
    assert any(not torch.equal(load("c", "model_2.pt")[k], mb[k]) for k in mb)
    assert not os.path.exists(os.path.join(base, "b", "train", "train_state.pt.tmp"))
    if mode == "eager":
        # today's command line: the same files as before, no state file, no (EMA) on the validation line
        files = os.listdir(os.path.join(base, "plain", "train"))
        assert "model_1.pt" in files and not any(f.startswith("train_state") for f in files), files
        assert "(EMA)" not in out["plain"] and not re.search(r"^resume:", out["plain"], flags=re.M)
        assert re.search(r"Finish valid \[1/1\]\. PSNR: [-\d.]+dB\n", out["plain"])
