"""What test.py and train.py print and write on a toy data folder, as SHA-256 sums: two trees behave alike iff their sums are equal
(docs/experiments/entry_points_share.md).

  python scripts/entry_points_dump.py [--tree DIR] [--keep DIR] [--only PREFIX[,PREFIX...]]

In a temporary folder: two seeded 48 x 40 HR PNGs with their x4 LR images (as test, training and validation set), a seeded
64-channel, 2-block x4 generator, a toy NIQE model of 16-pixel blocks and LpipsModel.random.  Then test.py six times (LR only, with
--niqe, --from_hr, with every score, the classical degradation with noise, jitter and JPEG, bicubic with JPEG 4:4:4) and train.py
twice (--synthetic with every --valid_* flag; a folder run with --lr_from_hr, the GPU pipeline and the whole degradation chain), then
train.py on HR patches of 32 with the optional terms of the generator's loss (docs/experiments/loss_terms.md): --phase train eager with
none, each one alone and all four, --phase pretrain with the SSIM term, and the all-four run captured (--hip_graph true); each
in a process of its own whose torch seed is set first.  --only runs the runs whose names begin with one of the prefixes.  --tree DIR takes test.py, train.py, utils.py and pesr_amd from another
checkout (for instance the parent commit's Python files, with PESR_HIP_LIB naming this tree's library); everything else comes from
this one.  Per run one JSON line: the exit code, the sum of stdout, of every PNG and checkpoint written, and of a checkpoint's tensors.
--keep DIR also writes every run's stdout there.  A run that fails ends the script.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", type=str, default=HERE)
ap.add_argument("--keep", type=str, default="")
ap.add_argument("--only", type=str, default="")
ARGS = ap.parse_args()
TREE = os.path.abspath(ARGS.tree)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

# the program runs as __main__ with its own folder in front of the path, after the seed
LAUNCH = ("import runpy, sys, torch; torch.manual_seed(0); prog = sys.argv[1]; sys.argv = sys.argv[1:]; "
          "sys.path.insert(0, {tree!r}); runpy.run_path(prog, run_name='__main__')")
NET = ["--num_channels", "64", "--num_blocks", "2"]
TEST = ["--dataset", "Toy", "--perceptual_model", "g.pt"] + NET
HR = TEST + ["--from_hr", "true"]
TRAIN = ["--phase", "pretrain", "--pretrained_model", "g.pt", "--batch_size", "4"] + NET
TOY32 = ["--pretrained_model", "g.pt", "--batch_size", "4", "--synthetic", "16", "--patch_size", "8", "--num_epochs", "2", "--snapshot_every", "1"] + NET
GAN = TOY32 + ["--phase", "train", "--hip_graph", "false"]
LPIPS, SSIM, TEXTURE, CX = ["--alpha_lpips", "1", "--lpips_loss", "w.pt"], ["--alpha_ssim", "1"], ["--alpha_texture", "1", "--texture_patch", "8"], ["--alpha_cx", "1"]
RUNS = [
    ("test_lr_only", "test.py", TEST),
    ("test_lr_only_niqe", "test.py", TEST + ["--niqe", "m.npz"]),
    ("test_from_hr", "test.py", HR),
    ("test_every_score", "test.py", HR + ["--ssim", "true", "--shave", "-1", "--niqe", "m.npz", "--lpips", "w.pt"]),
    ("test_classical", "test.py", HR + ["--degradation", "classical", "--blur_sigma", "1.6,0.8,0.5", "--noise_sigma", "5", "--resize_jitter", "0.7,box",
                                        "--jpeg_quality", "40"]),
    ("test_bicubic_jpeg444", "test.py", HR + ["--jpeg_quality", "60", "--jpeg_chroma", "444"]),
    ("train_synthetic", "train.py", TRAIN + ["--synthetic", "16", "--patch_size", "16", "--num_epochs", "2", "--valid_ssim", "true", "--valid_shave", "4",
                                             "--valid_niqe", "m.npz", "--valid_lpips", "w.pt"]),
    ("train_folder", "train.py", TRAIN + ["--train_dataset", "Toy", "--valid_dataset", "Toy", "--patch_size", "8", "--num_repeats", "4", "--lr_from_hr", "true",
                                          "--gpu_pipeline", "true", "--degradation", "classical", "--noise_sigma", "10", "--jpeg_quality", "30,95",
                                          "--resize_jitter", "0.5,2", "--max_iters", "2", "--num_epochs", "1"]),
    ("terms_none", "train.py", GAN),
    ("terms_lpips", "train.py", GAN + LPIPS),
    ("terms_ssim", "train.py", GAN + SSIM),
    ("terms_texture", "train.py", GAN + TEXTURE),
    ("terms_cx", "train.py", GAN + CX),
    ("terms_all", "train.py", GAN + LPIPS + SSIM + TEXTURE + CX),
    ("terms_pretrain_ssim", "train.py", TOY32 + ["--phase", "pretrain", "--hip_graph", "false"] + SSIM),
    ("terms_all_graph", "train.py", TOY32 + ["--phase", "train", "--hip_graph", "true"] + LPIPS + SSIM + TEXTURE + CX),
]
if ARGS.only:
    RUNS = [r for r in RUNS if r[0].startswith(tuple(ARGS.only.split(",")))]


def make_inputs(root):
    import warnings
    from PIL import Image
    from model import Generator
    from pesr_amd.lpips import LpipsModel
    from pesr_amd.niqe import NiqeModel
    rng = np.random.default_rng(2024)
    for k, name in enumerate(("a.png", "b.png")):
        yy, xx = np.mgrid[0:48, 0:40]
        base = np.kron(rng.integers(30, 226, (6, 5, 3)), np.ones((8, 8, 1)))
        hr = np.clip(np.rint(0.6 * base + (yy + 2 * xx)[..., None] * (0.5 + k) + rng.normal(0, 6, (48, 40, 3))), 0, 255).astype(np.uint8)
        lr = np.rint(hr.reshape(12, 4, 10, 4, 3).mean(axis=(1, 3))).astype(np.uint8)
        for part in ("test", "train", "valid"):
            for sub, im in (("HR", hr), ("LR", lr)):
                os.makedirs(os.path.join(root, "data", "origin", part, "Toy", sub), exist_ok=True)
                Image.fromarray(im).save(os.path.join(root, "data", "origin", part, "Toy", sub, name))
    torch.manual_seed(7)
    torch.save(Generator({"num_channels": 64, "depth": 2, "res_scale": 0.1, "scale": 4}).state_dict(), os.path.join(root, "g.pt"))
    NiqeModel(np.tile(np.array([2.5, 0.7] + [0.8, 0.0, 0.5, 0.5] * 4), 2), 0.04 * np.eye(36), 16).save(os.path.join(root, "m.npz"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        LpipsModel.random(5).save(os.path.join(root, "w.pt"))


def sha(data):
    return hashlib.sha256(data).hexdigest()


def tensors_sha(path):
    h = hashlib.sha256()
    for k, v in sorted(torch.load(path, map_location="cpu").items()):
        h.update(k.encode() + v.contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    root = tempfile.mkdtemp(prefix="entry_points_")
    make_inputs(root)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([TREE, HERE]))
    for name, prog, flags in RUNS:
        out = "out_" + name
        flags = flags + (["--save_path", out] if prog == "test.py" else ["--check_point", out])
        r = subprocess.run([sys.executable, "-c", LAUNCH.format(tree=TREE), os.path.join(TREE, prog)] + flags, cwd=root, env=env,
                           capture_output=True, text=True, timeout=420)
        if ARGS.keep:
            os.makedirs(ARGS.keep, exist_ok=True)
            with open(os.path.join(ARGS.keep, name + ".stdout"), "w") as fh:
                fh.write(r.stdout)
        files = {}
        for d, _, names in sorted(os.walk(os.path.join(root, out))):
            for f in sorted(names):
                p = os.path.join(d, f)
                if f.endswith((".png", ".pt")):
                    with open(p, "rb") as fh:
                        files[os.path.relpath(p, root)] = sha(fh.read())
                if f.endswith(".pt"):
                    files[os.path.relpath(p, root) + ":tensors"] = tensors_sha(p)
        print(json.dumps({"run": name, "rc": r.returncode, "stdout": sha(r.stdout.encode()), "stdout_lines": r.stdout.count("\n"), "files": files}),
              flush=True)
        if r.returncode != 0:
            sys.exit(name + " failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    print(json.dumps({"tree": TREE, "runs": len(RUNS)}))


if __name__ == "__main__":
    main()
