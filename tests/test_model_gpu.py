"""GPU parity of the drop-in `model` package + train steps vs golden vectors from the imported reference
(tests/golden/*.npz) and vs the CPU oracle.  Tolerances (stated on the 0..255 image scale):
G forward atol 2e-3 / rtol 1e-5; per-tensor grads max-abs error <= 1e-4 x max-abs of the reference grad;
scalar losses rtol 1e-5 (2e-5 after two optimizer steps)."""
import warnings

import numpy as np
import os
import pytest
import torch
import torch.nn.functional as F

from helpers import adam_close, close, dis_sd, gen_sd, load_golden, vgg_sd
from oracle import detrand
from oracle import model as OM
from oracle import step as OS

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message=".*pretrained vgg19.*")


def _G(C, depth, sd):
    from model import Generator
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1})
    G.load_state_dict(sd)
    return G.cuda()


def test_gv1_generator_small_fwd_bwd():
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    g = load_golden("gv1_generator_small")
    G = _G(16, 2, gen_sd(16, 2))
    assert list(G.state_dict().keys()) == [str(k) for k in g["keys"]]
    lr = detrand.image_batch((2, 3, 12, 12), 1234).cuda()
    hr = detrand.image_batch((2, 3, 48, 48), 1235).cuda()
    sr = G(lr)
    assert sr.shape == (2, 3, 48, 48)
    close(sr, g["sr"], 1e-5, 2e-3, "sr")
    loss = PF.l1_loss(nhwc(sr), nhwc(hr.contiguous(memory_format=torch.channels_last)))
    close(loss, g["loss"], 1e-5, what="l1")
    loss.backward()
    for k, p in G.named_parameters():
        close(p.grad, g["grad." + k], 1e-4, what="grad " + k)


def test_gv2_generator_full_sampled():
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    g = load_golden("gv2_generator_full")
    G = _G(256, 32, gen_sd(256, 32))
    lr = detrand.image_batch((2, 3, 48, 48), 1234).cuda()
    hr = detrand.image_batch((2, 3, 192, 192), 1235).cuda()
    sr = G(lr)
    flat = sr.contiguous().reshape(-1)            # logical NCHW order, as the golden indices
    close(flat[torch.from_numpy(g["sr_idx"]).cuda()], g["sr_val"], 1e-5, 2e-3, "sr samples")
    close(sr.sum(), g["sr_sum"], 1e-5, what="sr sum")
    loss = PF.l1_loss(nhwc(sr), nhwc(hr.contiguous(memory_format=torch.channels_last)))
    close(loss, g["loss"], 1e-5, what="l1")
    loss.backward()
    params = dict(G.named_parameters())
    for key in [k[5:] for k in g.files if k.startswith("gidx.")]:
        gr = params[key].grad.reshape(-1)[torch.from_numpy(g["gidx." + key]).cuda()]
        close(gr, g["gval." + key], 0.0, 1e-4 * float(g["gmax." + key]), "grad " + key)


def test_gv4_discriminator_small():
    from model import Discriminator
    g = load_golden("gv4_discriminator_small")
    D = Discriminator({"patch_size": 8, "spectral_norm": False})
    D.load_state_dict(dis_sd(8))
    D = D.cuda()
    a = detrand.image_batch((4, 3, 32, 32), 21).cuda()
    b = detrand.image_batch((4, 3, 32, 32), 22).cuda().requires_grad_(True)
    o1, o2 = D(a), D(b)
    close(o1, g["o1"], 2e-5, what="o1"); close(o2, g["o2"], 2e-5, what="o2")
    l = F.binary_cross_entropy_with_logits(o1 - o2, torch.ones(4, 1, device="cuda"))
    close(l, g["loss"], 1e-5, what="bce")
    l.backward()
    close(b.grad, g["gin"], 2e-4, what="grad input")
    for k, p in D.named_parameters():
        gr = p.grad.reshape(-1)[torch.from_numpy(g["gidx." + k]).cuda()]
        close(gr, g["gval." + k], 0.0, 2e-4 * float(g["gmax." + k]), "grad " + k)
    for k, v in D.state_dict().items():
        if "running" in k:
            close(v, g["buf." + k], 1e-4, what=k)
        elif "num_batches" in k:
            assert int(v) == 2


def test_gv7_vgg_small():
    from model import VGG
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    g = load_golden("gv7_vgg_small")
    V = VGG()
    assert sorted(V.state_dict().keys()) == sorted(str(k) for k in g["keys"])
    V.load_state_dict(vgg_sd())
    V = V.cuda()
    a = detrand.image_batch((2, 3, 32, 32), 31).cuda().requires_grad_(True)
    b = detrand.image_batch((2, 3, 32, 32), 32).cuda()
    fa, fb = V(a, b)
    close(fa, g["f_sr"], 2e-5, what="f_sr"); close(fb, g["f_hr"], 2e-5, what="f_hr")
    assert not fb.requires_grad
    m = PF.mse_loss(nhwc(fa), nhwc(fb))
    close(m, g["mse"], 2e-5, what="mse")
    m.backward()
    close(a.grad, g["gin"], 2e-4, what="grad input")


def test_vgg_shared_tail_equals_separate_passes():
    """VGG.forward runs conv4_1 .. conv5_4 of the sr and hr branches as ONE batch (functional.VggTailFn): features and the sr
    branch's input gradient must equal the two separate passes (reference model/vgg.py:24-26) to kernel-level precision - a
    per-image conv is the same arithmetic at batch B and 2B up to the split-K order the planner picks."""
    from model import VGG
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    V = VGG()
    V.load_state_dict(vgg_sd())
    V = V.cuda()
    x = detrand.image_batch((3, 3, 96, 64), 41).cuda()
    y = detrand.image_batch((3, 3, 96, 64), 42).cuda()
    res = []
    calls = []
    real = PF.VggTailFn.apply
    for merged in (True, False):
        a = x.clone().requires_grad_(True)
        if merged:
            PF.VggTailFn.apply = staticmethod(lambda *args: (calls.append(1), real(*args))[1])
        else:
            V.TAIL_START = 10 ** 6
        try:
            fa, fb = V(a, y)
        finally:
            PF.VggTailFn.apply = real
            V.TAIL_START = type(V).TAIL_START
        assert fa.shape == (3, 512, 6, 4) and not fb.requires_grad and fa.requires_grad
        PF.mse_loss(nhwc(fa), nhwc(fb)).backward()
        res.append((fa.detach().clone(), fb.clone(), a.grad.clone()))
    assert calls == [1]
    close(res[0][0], res[1][0], 1e-5, what="features(sr)")
    close(res[0][1], res[1][1], 1e-5, what="features(hr)")
    close(res[0][2], res[1][2], 2e-5, what="d mse / d sr")


def _trainer(C, depth, ps, lr=5e-5):
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    G = Generator({"num_channels": C, "depth": depth, "res_scale": 0.1}); G.load_state_dict(gen_sd(C, depth)); G.cuda()
    D = Discriminator({"patch_size": ps, "spectral_norm": False}); D.load_state_dict(dis_sd(ps)); D.cuda()
    V = VGG(); V.load_state_dict(vgg_sd()); V.cuda()
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=lr, betas=(0.9, 0.999))
    oD = FlatAdam(D.parameters(), lr=lr, betas=(0.9, 0.999))
    return Trainer(G, D, V, oG, oD), G, D


def test_gv8_two_gan_steps_vs_reference():
    """Two full GAN steps (losses + post-Adam parameters) against the run made with the reference's modules."""
    g = load_golden("gv8_gan_steps_small")
    tr, G, D = _trainer(16, 2, 8)
    for it in range(2):
        lr = detrand.image_batch((4, 3, 8, 8), 100 + it).cuda()
        hr = detrand.image_batch((4, 3, 32, 32), 200 + it).cuda()
        log = tr.gan_step(lr, hr)
        got = [float(log[k]) for k in ("l1", "vgg", "g", "tv", "d")]
        # step 0: 5e-5.  step 1 goes through two Adam updates, whose m/sqrt(v) normalisation amplifies summation-order
        # noise: the reference's OWN fp32-vs-fp64 difference at step 1 is 1.5e-4 of the largest loss (measured with
        # the oracle), so the honest bound there is a small multiple of that floor.
        close(np.array(got), g["losses"][it], 5e-5 if it == 0 else 5e-4, what=f"losses step {it}")
    for k, v in G.state_dict().items():
        adam_close(v.reshape(-1)[torch.from_numpy(g["G.idx." + k]).cuda()], g["G.val." + k], 5e-5, 2, "G." + k)
    for k, v in D.state_dict().items():
        if "running" in k or "num_batches" in k:
            # BN running stats after 8 forwards through Adam-perturbed weights (exact single-pass check: GV4)
            close(v.reshape(-1).float()[torch.from_numpy(g["D.idx." + k]).cuda()], g["D.val." + k], 2e-3, what="D." + k)
        else:
            adam_close(v.reshape(-1)[torch.from_numpy(g["D.idx." + k]).cuda()], g["D.val." + k], 5e-5, 2, "D." + k)


@pytest.mark.parametrize("B", [4, 16])
def test_paired_classifier_step_is_bit_identical_to_four_separate_calls(B):
    """Trainer.gan_step runs D's classifier ONCE per phase on [hr; sr] (Discriminator.classify: the classifier has no BatchNorm, its rows
    are independent; reference model/pesr.py:77-81 called four times per step, train.py:199-244).  The Linear kernels add rows in groups of
    sixteen and a shorter batch is padded with zero rows, so the paired step must leave EXACTLY what the four separate calls leave: losses,
    every parameter, BatchNorm running statistics - two steps, i.e. through both optimizers twice.  (Batches above 16 take the plain path.)"""
    res = []
    for pair in (True, False):
        tr, G, D = _trainer(16, 2, 8)
        tr.pair_classifier = pair
        logs = []
        for it in range(2):
            lr = detrand.image_batch((B, 3, 8, 8), 300 + it).cuda()
            hr = detrand.image_batch((B, 3, 32, 32), 400 + it).cuda()
            log = tr.gan_step(lr, hr)
            logs.append([float(log[k]) for k in ("l1", "vgg", "g", "tv", "d")])
        res.append((logs, {k: v.clone() for k, v in G.state_dict().items()}, {k: v.clone() for k, v in D.state_dict().items()}))
    (la, ga, da), (lb, gb, db) = res
    assert la == lb, (la, lb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), "G." + k
    for k in da:
        assert torch.equal(da[k], db[k]), "D." + k


def test_pretrain_step_vs_oracle():
    from model import Generator
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    sd = gen_sd(64, 3)
    G = Generator({"num_channels": 64, "depth": 3, "res_scale": 0.1}); G.load_state_dict(sd); G.cuda()
    tr = Trainer(G, optim_G=FlatAdam(G.parameters(), lr=1e-4))
    st = OS.TrainState(sd, None, None, {"depth": 3, "res_scale": 0.1, "learning_rate": 1e-4})
    for it in range(2):
        lr = detrand.image_batch((2, 3, 24, 24), 300 + it)
        hr = detrand.image_batch((2, 3, 96, 96), 400 + it)
        ref = OS.pretrain_step(st, lr, hr)
        log = tr.pretrain_step(lr.cuda(), hr.cuda())
        close(log["l1"], np.float32(ref["l1"]), 2e-5, what=f"l1 step {it}")
    for k, v in G.state_dict().items():
        adam_close(v, st.g[k], 1e-4, 2, k)


def test_state_dict_roundtrip_and_no_cpu_path():
    from model import Generator
    sd = gen_sd(64, 1)
    G = Generator({"num_channels": 64, "depth": 1, "res_scale": 0.1})
    G.load_state_dict(sd)
    for k, v in G.state_dict().items():
        assert torch.equal(v, sd[k]) and v.shape == sd[k].shape
    with pytest.raises(Exception, match="no CPU fallback"):
        G(torch.zeros(1, 3, 8, 8))


def test_generator_ragged_image_and_x8_ensemble():
    """Validation / test.py path: batch 1, arbitrary H x W (partial tiles everywhere), x8 self-ensemble on device."""
    import importlib.util, os
    from oracle import image as OI
    spec = importlib.util.spec_from_file_location("entry_test", os.path.join(os.path.dirname(os.path.dirname(__file__)), "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    sd = gen_sd(64, 2)
    G = _G(64, 2, sd)
    img = detrand.image_batch((1, 3, 37, 53), 77)
    with torch.no_grad():
        sr = G(img.cuda())
        ref = OM.generator_forward(sd, img, 2, 0.1)
        close(sr, ref, 1e-5, 2e-3, "ragged sr")
        ens = T.x8_forward(img.cuda(), G)
        ens_ref = OI.x8_forward(img, lambda t: OM.generator_forward(sd, t, 2, 0.1))
        close(ens, ens_ref, 1e-5, 2e-3, "x8 ensemble")


def test_x8_ensemble_on_device_vs_the_reference_fixture_gv10():
    """test.py's device-side x8 self-ensemble against golden GV10: outputs of the reference's OWN x8_forward (reference
    test.py:45-74) on a non-equivariant toy model whose arithmetic is exact in fp32 - bit for bit."""
    import importlib.util, os
    from helpers import x8_toy_model
    spec = importlib.util.spec_from_file_location("entry_test", os.path.join(os.path.dirname(os.path.dirname(__file__)), "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    g = load_golden("gv10_x8")
    model = x8_toy_model(g["weight_seed"], g["bias_seed"], "cuda")
    with torch.no_grad():
        for i, (shape, seed) in enumerate(zip(g["shapes"], g["seeds"])):
            img = detrand.image_batch(tuple(int(v) for v in shape), int(seed)).cuda()
            out = T.x8_forward(img, model)
            assert out.is_cuda and torch.equal(out.cpu(), torch.from_numpy(g[f"out{i}"])), i


def test_gv2c_generator_full_batch1():
    """Reference Generator 256 ch x 32 blocks (model/pesr.py:28-38) at [1,3,48,48] -> [1,3,192,192] - the shape of reference
    test.py:100-106 / BASELINE config 1.  At batch 1 the body layers have 16 pixel tiles: they run on the
    small-layer dispatch (split-K / direct kernels), which no batch-2 or batch-16 golden reaches."""
    from pesr_amd import functional as PF
    from pesr_amd.model.basic import nhwc
    g = load_golden("gv2c_generator_full_b1")
    G = _G(256, 32, gen_sd(256, 32))
    lr = detrand.image_batch((1, 3, 48, 48), 1234).cuda()
    hr = detrand.image_batch((1, 3, 192, 192), 1235).cuda()
    with torch.no_grad():
        sr0 = G(lr)                                           # the inference call of test.py
    sr = G(lr)
    assert torch.equal(sr0, sr.detach())
    flat = sr.contiguous().reshape(-1)
    idx = torch.from_numpy(g["sr_idx"]).cuda()
    close(flat[idx], g["sr_val"], 1e-5, 2e-3, "sr samples")
    close(flat[idx], g["sr_val64"], 1e-5, 2e-3, "sr samples vs fp64")
    close(sr.sum(), g["sr_sum"], 1e-5, what="sr sum")
    close(sr.abs().sum(), g["sr_abs_sum"], 1e-5, what="sr abs sum")
    loss = PF.l1_loss(nhwc(sr), nhwc(hr.contiguous(memory_format=torch.channels_last)))
    close(loss, g["loss"], 1e-5, what="l1")
    loss.backward()
    params = dict(G.named_parameters())
    errs = {}
    for key in [k[5:] for k in g.files if k.startswith("gidx.")]:
        gr = params[key].grad.reshape(-1)[torch.from_numpy(g["gidx." + key]).cuda()]
        close(gr, g["gval." + key], 0.0, 1e-4 * float(g["gmax." + key]), "grad " + key)          # SURVEY 8c's bar
        errs[key] = float((gr.double().cpu() - torch.from_numpy(g["g64." + key])).abs().max()) / float(g["gmax64." + key])
    worst = max(errs, key=errs.get)
    print(f"GV2c: worst gradient error vs fp64 {errs[worst]:.2e} ({worst}); the reference's own fp32: {float(g['floor_worst']):.2e}")
    assert errs[worst] <= 1e-4


def test_train_entrypoint_runs(tmp_path):
    """train.py end to end (pretrain, train from the pretrained checkpoint, train with --hip_graph true) in a FRESH interpreter:
    its DataLoader workers are forked, and forking this test process - tens of GB of mappings after the tests before it - took
    ~10 s per worker (139 s for this test; 7 s of it the entry point itself)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck, ckg = str(tmp_path / "ck"), str(tmp_path / "ck_graph")
    prog = f"""
import importlib.util, os, sys
sys.path.insert(0, {root!r})
spec = importlib.util.spec_from_file_location("entry_train", os.path.join({root!r}, "train.py"))
Tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(Tm)
def common(ck, iters):
    return ["--synthetic", "16", "--num_channels", "64", "--num_blocks", "2", "--patch_size", "8", "--batch_size", "4",
            "--num_epochs", "1", "--max_iters", str(iters), "--check_point", ck, "--snapshot_every", "1"]
Tm.main(common({ck!r}, 2) + ["--phase", "pretrain"])
best = os.path.join({ck!r}, "pretrain", "best_model.pt")
assert os.path.exists(best)
Tm.main(common({ck!r}, 2) + ["--phase", "train", "--pretrained_model", best])
# --hip_graph: two iterations eager, then the captured step replayed twice (bit-equality of replay and eager is pinned at
# Trainer level in test_gan_step_hipgraph_replay_is_bit_identical_to_eager; D is initialised unseeded here, as in the
# reference, so two runs of the entry point are not comparable)
Tm.main(common({ckg!r}, 4) + ["--phase", "train", "--pretrained_model", best, "--hip_graph", "true"])
print("ENTRY_OK")
"""
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "ENTRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "ck" / "pretrain" / "best_model.pt").exists()
    sd = torch.load(tmp_path / "ck" / "train" / "model_1.pt", map_location="cpu")
    assert list(sd.keys()) == list(OM.generator_shapes(64, 2).keys())      # the reference's checkpoint schema
    sdg = torch.load(tmp_path / "ck_graph" / "train" / "model_1.pt", map_location="cpu")
    assert list(sdg.keys()) == list(sd.keys()) and all(bool(torch.isfinite(v).all()) for v in sdg.values())
    assert any(not torch.equal(sdg[k], sd[k]) for k in sd)                  # it trained


def test_bench_py_plain_full_and_dumped_outputs(tmp_path):
    """bench.py at a toy size, in fresh interpreters: a plain run times exactly --steps steps and reports the headline only;
    --dump-outputs gives the same arrays in a second plain run and in a --full run (which adds the CPU oracle's parity check,
    kernel events and the matrix-pipe tally without changing what the steps compute)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    toy = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4", "--patch_size", "16", "--num_channels", "64", "--num_blocks", "2"]

    def bench(tag, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + toy + ["--dump-outputs", str(tmp_path / tag)] + list(extra),
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    a, b, f = bench("a"), bench("b"), bench("f", "--full", "--no-side")
    for d in (a, b, f):
        assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "patches/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-3 * d["value"]
    for k in ("cpu_baseline", "parity_check", "roofline", "step_flops", "host_enqueue_ms", "side"):
        assert k not in a, k
    assert f["parity_check"]["ok"] and "cpu_baseline" in f and "step_flops" in f and "host_enqueue_ms" in f
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == sorted(os.listdir(tmp_path / "f"))
    assert {"loss_d.npy", "loss_g.npy", "G.body.0.body.0.weight.npy", "D.classifier.0.weight.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        x = np.load(tmp_path / "a" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        for other in ("b", "f"):
            y = np.load(tmp_path / other / n)
            np.testing.assert_allclose(y, x, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(x).max(initial=0.0))), err_msg=f"{other}/{n}")
    assert float(np.load(tmp_path / "a" / "loss_d.npy")) == a["losses"]["d"]


def test_config5_large_tiles_64bit_indexing():
    """BASELINE config 5: G forward on 4 x 512x512 LR tiles (256 ch x 32 blocks).  The 256ch @ 2048^2 x 4 tensor has
    4.29e9 elements (> 2^31), so this exercises the 64-bit offsets.  Size-independent property: every output pixel
    accumulates its taps / channels in a fixed order whatever the tiling, so the interior rows of the full result equal the
    result on a full-width STRIP of rows (margin >= the 69-LR-pixel receptive field) BIT FOR BIT.
    (Rows, not a 2-D crop: along y the Winograd kernels apply the three taps directly and the receptive field is exact.
    Along x the F(4,3) transform reads six columns for four outputs; the two extra ones cancel exactly in real arithmetic
    but not in their last fp32 bits, so a crop boundary in x perturbs rounding up to 4 px per layer away - checked below
    against a tolerance instead.)"""
    G = _G(256, 32, gen_sd(256, 32))
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (4, 3, 512, 512), generator=g).float().cuda()
    with torch.no_grad():
        y = G(x)
        assert y.shape == (4, 3, 2048, 2048) and bool(torch.isfinite(y).all())
        m, (y0, s) = 72, (176, 240)
        yc = G(x[3:4, :, y0:y0 + s, :].contiguous())
        a = y[3, :, 4 * (y0 + m):4 * (y0 + s - m), :]
        b = yc[0, :, 4 * m:4 * (s - m), :]
        assert a.shape == b.shape == (3, 384, 2048)
        assert torch.equal(a, b), float((a - b).abs().max())
        # and the first image's top rows (zero padding included) against a top strip
        yc0 = G(x[0:1, :, :s, :].contiguous())
        assert torch.equal(y[0, :, :4 * (s - m), :], yc0[0, :, :4 * (s - m), :])
        # a 2-D crop: equal up to fp32 rounding (G-forward tolerance of the parity tests: 2e-3 on the 0..255 scale)
        x0 = 200
        yq = G(x[3:4, :, y0:y0 + s, x0:x0 + s].contiguous())
        a = y[3, :, 4 * (y0 + m):4 * (y0 + s - m), 4 * (x0 + m):4 * (x0 + s - m)]
        b = yq[0, :, 4 * m:4 * (s - m), 4 * m:4 * (s - m)]
        assert float((a - b).abs().max()) <= 2e-3


@pytest.mark.parametrize("gan_type,focal", [("SGAN", False), ("SGAN", True), ("RSGAN", False), ("RaSGAN", True), ("RaSGAN", False)])
def test_gan_step_other_branches_vs_oracle(gan_type, focal):
    """The non-default branches of reference train.py:210-213,244-253 (SGAN, plain BCE generator loss), one step."""
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    g_sd, d_sd, v_sd = gen_sd(64, 1), dis_sd(8), vgg_sd()
    G = Generator({"num_channels": 64, "depth": 1, "res_scale": 0.1}); G.load_state_dict(g_sd); G.cuda()
    D = Discriminator({"patch_size": 8, "spectral_norm": False}); D.load_state_dict(d_sd); D.cuda()
    V = VGG(); V.load_state_dict(v_sd); V.cuda()
    tr = Trainer(G, D, V, FlatAdam(G.parameters(), lr=5e-5), FlatAdam(D.parameters(), lr=5e-5), gan_type=gan_type,
                 focal_loss=focal, alpha_l1=0.5)
    st = OS.TrainState(g_sd, d_sd, v_sd, {"depth": 1, "res_scale": 0.1, "learning_rate": 5e-5, "gan_type": gan_type,
                                           "focal_loss": focal, "alpha_l1": 0.5})
    lr = detrand.image_batch((4, 3, 8, 8), 500); hr = detrand.image_batch((4, 3, 32, 32), 501)
    ref = OS.gan_step(st, lr, hr)
    log = tr.gan_step(lr.cuda(), hr.cuda())
    for k in ("l1", "vgg", "g", "tv", "d"):
        assert float(log[k]) == pytest.approx(ref[k], rel=5e-5, abs=1e-7), k
    for k, v in G.state_dict().items():
        adam_close(v, st.g[k], 5e-5, 1, "G." + k)


def test_test_entrypoint_end_to_end(tmp_path, monkeypatch):
    """test.py main() (reference test.py:76-116) on a folder of PNGs: perceptual model + x8-ensembled PSNR model blended
    in image space, written as PNG - against the CPU oracle's plumbing run on the same files (at most one grey level apart:
    the blend is rounded to uint8)."""
    import importlib.util, os
    from PIL import Image
    from oracle import image as OI
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("entry_test_e2e", os.path.join(root, "test.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    monkeypatch.chdir(tmp_path)
    lr_dir = tmp_path / "data" / "origin" / "test" / "Toy" / "LR"
    lr_dir.mkdir(parents=True)
    imgs = {}
    for name, (h, w), seed in (("a.png", (21, 30), 1), ("b.png", (16, 16), 2)):
        arr = detrand.image_batch((h, w, 3), 900 + seed).numpy().astype(np.uint8)
        Image.fromarray(arr).save(lr_dir / name)
        imgs[name] = arr
    sd_perc, sd_psnr = gen_sd(64, 2, seed=3), gen_sd(64, 2, seed=4)
    torch.save(sd_perc, tmp_path / "perc.pt"); torch.save(sd_psnr, tmp_path / "psnr.pt")
    T.main(["--dataset", "Toy", "--perceptual_model", str(tmp_path / "perc.pt"), "--psnr_model", str(tmp_path / "psnr.pt"),
            "--num_channels", "64", "--num_blocks", "2", "--alpha", "0.6", "--save_path", str(tmp_path / "out")])
    for name, arr in imgs.items():
        got = np.asarray(Image.open(tmp_path / "out" / "Toy" / name).convert("RGB")).astype(np.int32)
        x = torch.from_numpy(arr.transpose(2, 0, 1)[None].astype(np.float32))
        with torch.no_grad():
            ref = 0.6 * OM.generator_forward(sd_perc, x, 2, 0.1) + 0.4 * OI.x8_forward(x, lambda t: OM.generator_forward(sd_psnr, t, 2, 0.1))
        want = OI.tensor_to_img(ref).astype(np.int32)
        assert got.shape == want.shape == (4 * arr.shape[0], 4 * arr.shape[1], 3)
        assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.01, (np.abs(got - want).max(), (got != want).mean())


def test_config5_crop_vs_oracle():
    """BASELINE config 5 against the CPU oracle (not only against itself): the full 256 ch x 32 block generator on a 160x160 LR
    image (one 640x640 output; every layer takes the large-image tiling: several tiles per row and per column, the F(4,3)
    kernels' 96-px-wide tiles, ragged last tiles) - G-forward tolerance of SURVEY 8c."""
    sd = gen_sd(256, 32)
    G = _G(256, 32, sd)
    x = detrand.image_batch((1, 3, 160, 160), 55)
    with torch.no_grad():
        y = G(x.cuda())
        torch.set_num_threads(max(1, min(16, len(__import__("os").sched_getaffinity(0)))))
        ref = OM.generator_forward(sd, x, 32, 0.1)
    assert y.shape == ref.shape == (1, 3, 640, 640)
    close(y, ref, 1e-5, 2e-3, "config-5-style crop vs oracle")


def _ref_basic_block(cin, cout, stride, bias, bn, act):
    import torch.nn as nn
    m = [nn.Conv2d(cin, cout, 3, padding=1, stride=stride, bias=bias)]
    if bn:
        m.append(nn.BatchNorm2d(cout))
    if act is not None:
        m.append(act)
    return nn.Sequential(*m)


@pytest.mark.parametrize("bias,bn,act,train", [(True, True, "relu", True), (False, True, "lrelu", False), (True, False, "lrelu", True),
                                               (False, True, None, True), (True, True, "lrelu", False), (False, False, "relu", True)])
def test_basic_block_constructor_branches(bias, bn, act, train):
    """Every BasicBlock the reference's constructor accepts (model/basic.py:19-31): conv bias, BatchNorm on / off and in eval
    mode, ReLU / LeakyReLU / no activation - against the same nn.Sequential built from torch modules on the CPU."""
    import copy
    import torch.nn as nn
    from model import BasicBlock
    mk = lambda: {"relu": nn.ReLU(True), "lrelu": nn.LeakyReLU(0.2, True), None: None}[act]
    torch.manual_seed(3)
    blk = BasicBlock(32, 64, 3, stride=1, bias=bias, bn=bn, act=mk(), sn=False)
    ref = _ref_basic_block(32, 64, 1, bias, bn, mk())
    ref.load_state_dict(blk.state_dict())
    if bn:
        with torch.no_grad():
            for m in (blk[1], ref[1]):
                m.running_mean.copy_(detrand.uniform((64,), 5, -0.2, 0.2)); m.running_var.copy_(detrand.uniform((64,), 6, 0.5, 1.5))
                m.weight.copy_(detrand.uniform((64,), 7, 0.5, 1.5)); m.bias.copy_(detrand.uniform((64,), 8, -0.1, 0.1))
    blk.train(train); ref.train(train)
    blk = blk.cuda()
    x = detrand.uniform((2, 32, 12, 16), 11)
    xr = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
    gy = detrand.uniform((2, 64, 12, 16), 12)
    yr = ref(xr); yr.backward(gy)
    yg = blk(xg); yg.backward(gy.cuda())
    close(yg, yr.detach(), 2e-5, what="forward")
    close(xg.grad, xr.grad, 1e-4, what="grad input")
    for (k, pg), (_, pr) in zip(blk.named_parameters(), ref.named_parameters()):
        if bn and train and k == "0.bias":      # a bias in front of training-mode BN has an exactly-zero gradient: compare absolutely
            assert float(pg.grad.abs().max()) <= 1e-4 * float(gy.abs().sum()) and float(pr.grad.abs().max()) <= 1e-4 * float(gy.abs().sum())
        else:
            close(pg.grad, pr.grad, 1e-4, what="grad " + k)
    if bn:
        close(blk[1].running_mean, ref[1].running_mean, 1e-5, what="running_mean"); close(blk[1].running_var, ref[1].running_var, 1e-5, what="running_var")


@pytest.mark.parametrize("cin,cout", [(64, 3), (3, 64)])
def test_basic_block_leaky_relu_with_a_three_channel_side(cin, cout):
    """BasicBlock(bn=False, act=LeakyReLU) into and out of three channels: the node behind it (ConvLReluFn) takes its weight and input
    gradients from the same routing as every other conv node, so the C -> 3 block has a weight gradient (it used to end in
    "unsupported shape": the general kernel refuses Cout % 4 != 0) - against the same nn.Sequential on the CPU."""
    import torch.nn as nn
    from model import BasicBlock
    torch.manual_seed(3)
    blk = BasicBlock(cin, cout, 3, bias=True, bn=False, act=nn.LeakyReLU(0.2, True), sn=False)
    ref = _ref_basic_block(cin, cout, 1, True, False, nn.LeakyReLU(0.2, True))
    ref.load_state_dict(blk.state_dict())
    blk = blk.cuda()
    x = detrand.uniform((2, cin, 12, 16), 11)
    xr = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
    gy = detrand.uniform((2, cout, 12, 16), 12)
    yr = ref(xr); yr.backward(gy)
    yg = blk(xg); yg.backward(gy.cuda())
    close(yg, yr.detach(), 2e-5, what="forward")
    close(xg.grad, xr.grad, 1e-4, what="grad input")
    for (k, pg), (_, pr) in zip(blk.named_parameters(), ref.named_parameters()):
        close(pg.grad, pr.grad, 1e-4, what="grad " + k)


@pytest.mark.parametrize("bias,bn,act", [(True, True, "relu"), (False, False, "relu"), (True, False, "lrelu")])
def test_res_block_constructor_branches(bias, bn, act):
    """ResBlock variants of reference model/basic.py:33-52 beyond the one the Generator uses (bn=True, bias=False, LeakyReLU)."""
    import torch.nn as nn
    from model import ResBlock
    mk = lambda: nn.ReLU(True) if act == "relu" else nn.LeakyReLU(0.1, True)
    torch.manual_seed(4)
    blk = ResBlock(64, 3, bias=bias, bn=bn, act=mk(), res_scale=0.3)
    body = []
    for i in range(2):
        body.append(nn.Conv2d(64, 64, 3, padding=1, bias=bias))
        if bn:
            body.append(nn.BatchNorm2d(64))
        if i == 0:
            body.append(mk())
    ref = nn.Sequential(*body)
    ref.load_state_dict(blk.body.state_dict())
    blk = blk.cuda()
    x = detrand.uniform((2, 64, 10, 12), 21)
    xr = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
    gy = detrand.uniform((2, 64, 10, 12), 22)
    yr = ref(xr).mul(0.3) + xr; yr.backward(gy)
    yg = blk(xg); yg.backward(gy.cuda())
    close(yg, yr.detach(), 2e-5, what="forward")
    close(xg.grad, xr.grad, 1e-4, what="grad input")
    for (k, pg), (_, pr) in zip(blk.body.named_parameters(), ref.named_parameters()):
        if bn and k.endswith("bias") and k[0] in "03" and pr.dim() == 1 and pr.shape[0] == 64 and "0.bias" == k or (bn and k == "3.bias"):
            continue                               # conv biases in front of training-mode BN: exactly-zero gradients
        close(pg.grad, pr.grad, 1e-4, what="grad " + k)


@pytest.mark.parametrize("k", [5, 1])
def test_res_block_other_kernel_size_vs_torch(k):
    """ResBlock(n_feats, kernel_size != 3) in the reference's default configuration (bias, no BN, ReLU; model/basic.py:33-52
    accepts any size): must take the un-fused generic-kernel path, never the 3x3 packers (a [C,C,5,5] weight read
    as [C,C,3,3] was silently wrong) - against the same block built from nn.Conv2d on the CPU."""
    import torch.nn as nn
    from model import ResBlock
    from pesr_amd import ops
    torch.manual_seed(5)
    blk = ResBlock(64, k, res_scale=0.1)
    assert not blk._fused
    ref = nn.Sequential(nn.Conv2d(64, 64, k, padding=k // 2), nn.ReLU(True), nn.Conv2d(64, 64, k, padding=k // 2))
    ref.load_state_dict(blk.body.state_dict())
    blk = blk.cuda()
    x = detrand.uniform((2, 64, 12, 16), 31)      # W % 4 == 0, C % 64 == 0: a shape the Winograd dispatch WOULD have taken
    xr = x.clone().requires_grad_(True); xg = x.cuda().requires_grad_(True)
    gy = detrand.uniform((2, 64, 12, 16), 32)
    yr = ref(xr).mul(0.1) + xr; yr.backward(gy)
    yg = blk(xg); yg.backward(gy.cuda())
    close(yg, yr.detach(), 2e-5, what="forward")
    close(xg.grad, xr.grad, 1e-4, what="grad input")
    for (kk, pg), (_, pr) in zip(blk.body.named_parameters(), ref.named_parameters()):
        close(pg.grad, pr.grad, 1e-4, what="grad " + kk)
    w5 = torch.zeros(64, 64, 5, 5, device="cuda")
    for pack in (ops.pack_conv3x3, ops.pack_conv3x3_wino, ops.pack_conv3x3_wino4, ops.pack_conv3x3_bf16):
        with pytest.raises(AssertionError, match="3x3"):
            pack(w5, 0)


def test_discriminator_second_order_forward_equals_forward():
    """Discriminator.forward_second_order (un-fused, twice differentiable) computes the same D(x) and the same first-order
    gradients as the fused forward."""
    from model import Discriminator
    sd = dis_sd(8)
    outs = []
    for second in (False, True):
        D = Discriminator({"patch_size": 8, "spectral_norm": False}); D.load_state_dict(sd); D = D.cuda()
        x = detrand.image_batch((4, 3, 32, 32), 21).cuda().requires_grad_(True)
        o = D.forward_second_order(x) if second else D(x)
        o.sum().backward()
        outs.append((o.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in D.named_parameters()}))
    close(outs[1][0], outs[0][0], 1e-5, what="D(x)")
    close(outs[1][1], outs[0][1], 2e-4, what="dD/dx")
    for k in outs[0][2]:
        if k != "classifier.2.bias":
            close(outs[1][2][k], outs[0][2][k], 2e-4, what="grad " + k)


def _gv11_float64_step():
    """The gradient-penalty step of test_gv11 by the CPU oracle (oracle/step.py) in float64, from the same weights and batch.
    -> (dD/dx at x_both [N, 3, H, W], D's parameter gradients, D's parameters after the Adam step, the number of BatchNorm / LeakyReLU
    inputs of D(x_both) with |z| < 1e-6)"""
    c = lambda sd: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    st = OS.TrainState(c(gen_sd(16, 2)), c(dis_sd(8)), c(vgg_sd()), {"depth": 2, "res_scale": 0.1, "learning_rate": 5e-5, "GP": True})
    lr = detrand.image_batch((4, 3, 8, 8), 100).double(); hr = detrand.image_batch((4, 3, 32, 32), 200).double()
    u = detrand.uniform((4, 1, 1, 1), 77, 0.0, 1.0).double()
    xb = (hr * u + st.G(lr).detach() * (1 - u)).requires_grad_(True)
    near, real = [0], F.leaky_relu

    def counted(h, slope=0.01, inplace=False):
        near[0] += int((h.detach().abs() < 1e-6).sum())
        return real(h, slope)
    F.leaky_relu = counted
    try:
        gx, = torch.autograd.grad(OM.discriminator_forward(dict(st.d), xb, update_running_stats=False).sum(), xb)
    finally:
        F.leaky_relu = real
    OS.gan_step(st, lr, hr, gp_u=u)
    return gx, {k: v.grad for k, v in st.d.items() if getattr(v, "grad", None) is not None}, {k: v.detach() for k, v in st.d.items()}, near[0]


def test_gv11_gradient_penalty_step_vs_reference():
    """--GP true (reference train.py:216-226): one D-phase with the gradient penalty - torch.autograd.grad(D(x_both), x_both,
    create_graph=True) and the backward THROUGH that gradient, all inside D on the HIP kernels - against the run made with the
    reference's own modules: total D loss, the penalty, dD/dx, D's gradients, post-Adam parameters.

    One BatchNorm output of features.2 is 4.4e-8 at x_both - below what fp32 resolves (u (|gamma xhat| + |beta|) is 1e-7 .. 1e-6 there),
    so its LeakyReLU branch is a coin toss for any fp32 evaluation.  The reference's fp32 run, which the golden file records, took the
    negative branch; float64 takes the positive one; dD/dx differs between the two by 2.4e-3 of its maximum and the gradient of
    features.2.1.bias by 8.6e-4 (docs/experiments/bn_tests.md).  It is the only such input of D(x_both) (asserted), so the golden file
    and the CPU oracle's float64 step are the two possible outcomes: the kernels must match ONE of them, the same one throughout, to
    the tolerances this test always had.  The loss and the penalty differ by less than 1e-7 between the two and are held to the
    golden file alone."""
    g = load_golden("gv11_gradient_penalty_small")
    gx64, grad64, par64, near = _gv11_float64_step()
    assert near == 1, near
    tr, G, D = _trainer(16, 2, 8)
    tr.gradient_penalty = True
    lr = detrand.image_batch((4, 3, 8, 8), 100).cuda()
    hr = detrand.image_batch((4, 3, 32, 32), 200).cuda()
    u = detrand.uniform((4, 1, 1, 1), 77, 0.0, 1.0).cuda()
    # dD/dx at the interpolate, on its own
    sr = G(lr).detach()
    hr_cl = hr.contiguous(memory_format=torch.channels_last)
    x_both = (hr_cl * u + sr * (1 - u)).detach().requires_grad_(True)
    import copy
    D2 = copy.deepcopy(D)
    gx = torch.autograd.grad(D2.forward_second_order(x_both).sum(), x_both)[0]
    got = gx.contiguous().reshape(-1)[torch.from_numpy(g["gx_idx"]).cuda()].double().cpu().numpy()
    errs = [float(np.abs(got - g["gx_val"]).max()), float(np.abs(got - gx64.reshape(-1)[torch.from_numpy(g["gx_idx"])].numpy()).max())]
    print("dD/dx_both: max error against the golden file and against the float64 step:", errs)
    f64 = int(np.argmin(errs)) == 1                                  # which of the two outcomes the kernels took
    assert min(errs) <= 5e-4 * float(g["gx_max"]), f"dD/dx_both: max err {errs} against either outcome, scale {float(g['gx_max']):.3e}"
    log = tr.gan_step(lr, hr, gp_u=u)
    close(log["gp"], g["gp"], 5e-5, what="gradient penalty")
    close(log["d"], g["total"], 5e-5, what="total D loss")
    worst = 0.0
    for k, p in D.named_parameters():
        got = p.grad.reshape(-1)[torch.from_numpy(g["gidx." + k]).cuda()].double().cpu().numpy()
        want = grad64[k].reshape(-1)[torch.from_numpy(g["gidx." + k])].numpy() if f64 else g["gval." + k]
        err = np.abs(got - want).max() / (float(g["gmax." + k]) + 1e-30)
        worst = max(worst, err)
        assert err <= 1e-4, f"grad {k}: {err:.2e} of the maximum"         # measured: 6e-6
    print(f"worst D gradient error with the penalty: {worst:.2e} of a tensor's maximum")
    for k, v in D.state_dict().items():
        if "num_batches" in k:
            assert int(v) == 5
        elif "running" not in k:
            want = par64[k].reshape(-1)[torch.from_numpy(g["pidx." + k])].numpy() if f64 else g["pval." + k]
            adam_close(v.reshape(-1)[torch.from_numpy(g["pidx." + k]).cuda()], want, 5e-5, 1, "D." + k)


def test_gan_step_hipgraph_replay_is_bit_identical_to_eager():
    """Trainer.capture_gan_step: three replayed GAN steps (new batch each) leave the same losses and the same G / D parameters,
    bit for bit, as three eager steps from the same state - the two Adam steps read lr and the step count from device memory,
    so nothing step-dependent is baked into the captured launches.  Includes an lr change between replays (StepLR)."""
    tra, Ga, Da = _trainer(16, 2, 8)
    trb, Gb, Db = _trainer(16, 2, 8)
    data = [(detrand.image_batch((4, 3, 8, 8), 50 + i).cuda(), detrand.image_batch((4, 3, 32, 32), 60 + i).cuda()) for i in range(5)]
    for lr, hr in data[:2]:
        tra.gan_step(lr, hr); trb.gan_step(lr, hr)
    step = trb.capture_gan_step(*data[0])
    assert trb.optim_G.steps == tra.optim_G.steps == 2          # the capture itself executes nothing
    for i, (lr, hr) in enumerate(data[2:]):
        if i == 2:
            for t in (tra, trb):
                t.optim_G.param_groups[0]["lr"] *= 0.5; t.optim_D.param_groups[0]["lr"] *= 0.5
        la, lb = tra.gan_step(lr, hr), step(lr, hr)
        for k in la:
            assert la[k].item() == lb[k].item(), (i, k, la[k].item(), lb[k].item())
    assert trb.optim_G.steps == tra.optim_G.steps == 5
    for pa, pb in zip(list(Ga.parameters()) + list(Da.parameters()), list(Gb.parameters()) + list(Db.parameters())):
        assert torch.equal(pa, pb)
    # eager steps keep working after the capture (device-state Adam) and stay in lock-step
    la, lb = tra.gan_step(*data[0]), trb.gan_step(*data[0])
    assert la["d"].item() == lb["d"].item() and torch.equal(next(Ga.parameters()), next(Gb.parameters()))
    # the pretrain step (reference train.py:164-173) captured on the same trainer
    for lr, hr in data[:2]:
        tra.pretrain_step(lr, hr); trb.pretrain_step(lr, hr)
    pstep = trb.capture_pretrain_step(*data[0])
    for lr, hr in data[2:4]:
        assert tra.pretrain_step(lr, hr)["l1"].item() == pstep(lr, hr)["l1"].item()
    for pa, pb in zip(Ga.parameters(), Gb.parameters()):
        assert torch.equal(pa, pb)


def test_hipgraph_replay_then_forward_at_a_new_shape_uses_fresh_weights():
    """After replays, a packing that the captured step never built (validation runs G on full images of another shape and so
    on another kernel dispatch) must be made from the CURRENT weights: the replayed Adam kernels write through raw pointers,
    so Trainer._replay bumps the weight epochs and re-stamps only the packings the captured repack launches rebuild.  Twin
    trainers, one eager and one replaying; a forward at a new shape BEFORE the capture creates the packing that would
    otherwise be served stale afterwards."""
    tra, Ga, Da = _trainer(16, 2, 8)
    trb, Gb, Db = _trainer(16, 2, 8)
    data = [(detrand.image_batch((4, 3, 8, 8), 50 + i).cuda(), detrand.image_batch((4, 3, 32, 32), 60 + i).cuda()) for i in range(5)]
    probe = detrand.image_batch((1, 3, 10, 14), 77).cuda()       # width 14: not an F(4,3) shape -> F(2,3) / direct packings
    for lr, hr in data[:2]:
        tra.gan_step(lr, hr); trb.gan_step(lr, hr)
    with torch.no_grad():
        assert torch.equal(Ga(probe), Gb(probe))                 # builds the validation-shape packings from step-2 weights
    step = trb.capture_gan_step(*data[0])
    for lr, hr in data[2:]:
        tra.gan_step(lr, hr); step(lr, hr)
    Ga.eval(); Gb.eval()
    with torch.no_grad():
        ya, yb = Ga(probe), Gb(probe)
        assert torch.equal(ya, yb), float((ya - yb).abs().max())
        probe2 = detrand.image_batch((2, 3, 9, 6), 78).cuda()    # and a shape nobody has seen yet
        assert torch.equal(Ga(probe2), Gb(probe2))
        # D at another batch size as well (its classifier fixes the patch size)
        hr1 = data[0][1][:2].contiguous(memory_format=torch.channels_last)
        assert torch.equal(Da(hr1), Db(hr1))
    # and the packings of the captured shape are still served (no rebuild storm): one more replay stays in lock-step
    la, lb = tra.gan_step(*data[1]), step(*data[1])
    assert la["vgg"].item() == lb["vgg"].item()


def test_gradient_penalty_step_captured_as_hipgraph():
    """--GP steps replay too: the interpolation weights u (reference train.py:217) are a graph input."""
    from pesr_amd.step import Trainer
    tra, Ga, Da = _trainer(16, 2, 8)
    trb, Gb, Db = _trainer(16, 2, 8)
    tra.gradient_penalty = trb.gradient_penalty = True
    data = [(detrand.image_batch((4, 3, 8, 8), 50 + i).cuda(), detrand.image_batch((4, 3, 32, 32), 60 + i).cuda()) for i in range(4)]
    us = [torch.rand(4, 1, 1, 1, generator=torch.Generator().manual_seed(i)).cuda() for i in range(4)]
    for (lr, hr), u in zip(data[:2], us[:2]):
        tra.gan_step(lr, hr, gp_u=u); trb.gan_step(lr, hr, gp_u=u)
    step = trb.capture_gan_step(*data[0])
    for (lr, hr), u in zip(data[2:], us[2:]):
        la, lb = tra.gan_step(lr, hr, gp_u=u), step(lr, hr, gp_u=u)
        for k in la:
            assert la[k].item() == lb[k].item(), (k, la[k].item(), lb[k].item())
    for pa, pb in zip(list(Ga.parameters()) + list(Da.parameters()), list(Gb.parameters()) + list(Db.parameters())):
        assert torch.equal(pa, pb)
    lr, hr = data[0]
    assert "gp" in step(lr, hr)          # u drawn by the replay itself


def test_discriminator_with_spectral_norm_step_vs_oracle():
    """--spectral_norm true (reference model/basic.py:25 is a NameError there; torch.nn.utils.spectral_norm is what it means):
    one full GAN step with a spectrally normalised Discriminator against the CPU oracle - four D forwards with one power
    iteration each (u / v carried from call to call), D's update through weight_orig, losses, buffers, post-Adam parameters."""
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    g_sd, d_sd, v_sd = gen_sd(16, 1), dis_sd(8, spectral_norm=True), vgg_sd()
    G = Generator({"num_channels": 16, "depth": 1, "res_scale": 0.1}); G.load_state_dict(g_sd); G.cuda()
    D = Discriminator({"patch_size": 8, "spectral_norm": True})
    assert list(D.state_dict().keys()) == list(d_sd.keys())          # torch's spectral_norm schema, in torch's order
    D.load_state_dict(d_sd); D.cuda()
    V = VGG(); V.load_state_dict(v_sd); V.cuda()
    tr = Trainer(G, D, V, FlatAdam(G.parameters(), lr=5e-5), FlatAdam(D.parameters(), lr=5e-5))
    st = OS.TrainState(g_sd, d_sd, v_sd, {"depth": 1, "res_scale": 0.1, "learning_rate": 5e-5})
    for it in range(2):
        lr = detrand.image_batch((4, 3, 8, 8), 510 + it); hr = detrand.image_batch((4, 3, 32, 32), 520 + it)
        ref = OS.gan_step(st, lr, hr)
        log = tr.gan_step(lr.cuda(), hr.cuda())
        for k in ("l1", "vgg", "g", "tv", "d"):
            assert float(log[k]) == pytest.approx(ref[k], rel=5e-5 if it == 0 else 5e-4, abs=1e-7), (it, k)
    got = D.state_dict()
    for k, v in st.d.items():
        if k.endswith(("weight_u", "weight_v")):
            close(got[k], v, 2e-4, what=k)                           # eight power iterations in, still the same vectors
        elif v.is_floating_point() and "running" not in k:
            adam_close(got[k], v, 5e-5, 2, "D." + k)
    for k, v in G.state_dict().items():
        adam_close(v, st.g[k], 5e-5, 2, "G." + k)
