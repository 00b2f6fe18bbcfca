#!/usr/bin/env python3
"""Headline benchmark: HR-patches/sec of the x4 SR GAN train step (48 -> 192) on N MI355X of one node.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one full GAN train step of reference train.py:194-259 (G forward, 4 D forwards, 2 VGG passes,
RSGAN + focal losses, D and G backward, both Adam updates) on a per-GPU batch of 16 synthetic
DIV2K-shaped crops (LR 48x48, HR 192x192, integers 0..255 as fp32) already resident in HBM.  Weak scaling:
per-GPU batch fixed, global batch 16*N, gradients all-reduced over RCCL inside the optimizers.
Rank 0 prints ONE JSON line.  See DESIGN.md "Measurement" for the roofline / cpu_baseline / parity_check definitions.
`python bench.py --gpus N` without a launcher environment starts the N ranks itself (torch.distributed.run as a child
process, before this process touches a GPU); it exits non-zero rather than report fewer GPUs than asked for.

A plain run sets up, warms up, times --steps steps and prints the headline line.  Everything else it can measure or check
(CPU baseline and parity check, side measurements, roofline kernel events, the matrix-pipe tally, host enqueue time,
per-collective and exposed-communication timing, the peer-copy engine probe, the replica check) runs only with --full.
--dump-outputs DIR writes what the last timed step computed (losses, and the networks' state after it) as .npy files.
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32-input MFMA
PEAK_BF16_MFMA_TFLOPS = 2500.0        # same guide: dense bf16 MFMA (the denominator of the optional --precision bf16 row)
GFLOP_PER_PATCH = {"gan": 844.10, "pretrain": 694.69}   # SURVEY.md 8(d), necessary work per HR patch
K1_GFLOP = 2.0 * 16 * 48 * 48 * 256 * 256 * 9 / 1e9     # body conv 256->256 @48x48, batch 16: 43.487 GFLOP per launch


PMC_SUMMARIES = ("r06_k1_pmc_summary.csv", "r05_k1_pmc_summary.csv", "r04_k1_pmc_summary.csv", "r04_bf16_pmc_summary.csv", "r03_k1_pmc_summary.csv", "r03_bf16_pmc_summary.csv")     # newest first
# kernel name -> the source file whose hash must match the summary's side-car (scripts/summarize_profiles.py writes <summary>.meta.json)
KERNEL_SOURCE = {"conv3x3_bf16x3_kernel": "conv3x3_bf16x3.hip", "conv3x3_wino4_kernel": "conv3x3_wino4.hip", "conv3x3_wino_kernel": "conv3x3_wino.hip", "conv3x3_mfma_kernel": "conv3x3_mfma.hip",
                 "conv3x3_wgrad_wino4p_kernel": "conv3x3_wgrad_wino4.hip", "conv3x3_wgrad_wino4x_kernel": "conv3x3_wgrad_wino4.hip", "conv3x3_wgrad_wino4_kernel": "conv3x3_wgrad_wino4.hip",
                 "conv3x3_wgrad_wino_kernel": "conv3x3_wgrad_wino.hip", "conv3x3_wgrad_kernel": "conv3x3_wgrad.hip",
                 "conv3x3_bf16_kernel": "conv3x3_bf16.hip", "conv3x3_wgrad_bf16_kernel": "conv3x3_wgrad_bf16.hip"}


def k1_hbm_traffic_bytes(kernel_substr):
    """HBM bytes per launch of a body-shape kernel from the committed rocprofv3 --pmc passes (bench.py cannot read PMCs
    live): 2 x FETCH_SIZE (gfx950 correction, MI355X_MICROARCH.md "HBM") + WRITE_SIZE, both in KiB in the profile.  A summary
    is used only if its side-car says it was taken on the CURRENT source of that kernel (sha256 of the .hip file); a stale or
    un-stamped one is refused.  -> (bytes | None, file name | None, sha256[:16] of the kernel source | reason)"""
    import csv
    import hashlib
    srcfile = KERNEL_SOURCE.get(kernel_substr.split("<")[0].strip())
    try:
        cur = hashlib.sha256(open(os.path.join(ROOT, "pesr_amd", "csrc", srcfile), "rb").read()).hexdigest() if srcfile else None
    except OSError:
        cur = None
    why = "no committed PMC summary found"
    for name in PMC_SUMMARIES:
        path = os.path.join(ROOT, "profiles", name)
        try:
            fetch = write = None
            for r in csv.DictReader(open(path)):
                if kernel_substr in r["kernel"]:
                    if r["counter"] == "FETCH_SIZE":
                        fetch = float(r["mean_per_launch"])
                    elif r["counter"] == "WRITE_SIZE":
                        write = float(r["mean_per_launch"])
            if not (fetch and write):
                continue
            try:
                stamped = json.load(open(os.path.splitext(path)[0] + ".meta.json"))["sources_sha256"].get(srcfile)
            except (OSError, KeyError, ValueError):
                stamped = None
            if cur is None or stamped != cur:
                why = f"profiles/{name} is stale: it was not taken on the current {srcfile} (re-run scripts/gpu_job.sh pmc)"
                continue
            return int((2 * fetch + write) * 1024), name, cur[:16]
        except OSError:
            continue
    return None, None, why


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) with no launcher environment: start one process per GPU.  Runs BEFORE this
    process makes any HIP call (device_count() does not initialise the GPU on this image) and never execs."""
    import socket
    import subprocess
    n_vis = torch.cuda.device_count()
    if n_vis < args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_vis} GPU(s) visible on this node")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # the host driver supports dmabuf IPC only
    raise SystemExit(subprocess.call(cmd, env=env))


def build(args, device, world):
    from model import Discriminator, Generator, VGG
    from pesr_amd.optim import FlatAdam
    from pesr_amd.step import Trainer
    torch.manual_seed(0)
    opt = {"patch_size": args.patch_size, "num_channels": args.num_channels, "depth": args.num_blocks,
           "res_scale": 0.1, "spectral_norm": False}
    G = Generator(opt).to(device)
    D = vgg = oD = None
    if args.workload == "gan":
        D = Discriminator(opt).to(device)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vgg = VGG().to(device)
        oD = FlatAdam(D.parameters(), lr=args.lr, betas=(0.9, 0.999))
    oG = FlatAdam([p for p in G.parameters() if p.requires_grad], lr=args.lr, betas=(0.9, 0.999))
    if world > 1:   # identical replicas: broadcast rank 0's initial weights once
        dist.broadcast(oG.flat.flat_p, 0)
        if oD is not None:
            dist.broadcast(oD.flat.flat_p, 0)
    return Trainer(G, D, vgg, oG, oD, world_size=world), G, D, vgg


def synth_batch(batch, patch, seed, device):
    g = torch.Generator().manual_seed(seed)
    lr = torch.randint(0, 256, (batch, 3, patch, patch), generator=g).float()
    hr = torch.randint(0, 256, (batch, 3, 4 * patch, 4 * patch), generator=g).float()
    return lr.to(device), hr.to(device)


def host_cores() -> int:
    """Cores this process may really use: CPU affinity capped by the cgroup CPU quota (the GPU box exposes 256
    logical CPUs under a 16-CPU quota; oversubscribing torch's pool there is 50x slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


DUMP_SAMPLE = 1 << 16           # --dump-outputs: elements kept per tensor (larger ones: a fixed, seeded sample)
DUMP_LIMIT_BYTES = 64 << 20


def dump_sample(t, name, n=DUMP_SAMPLE):
    """float32 numpy copy of `t` flattened: all of it, or `n` elements at positions drawn from a generator seeded by `name`
    (sorted; the same positions in every run)."""
    import zlib
    flat = t.detach().reshape(-1)
    if flat.numel() > n:
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        idx = torch.randint(0, flat.numel(), (n,), generator=g).sort().values
        flat = flat[idx.to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(path, arrays):
    """arrays: [(name, numpy array)] -> path/<name>.npy; refuses to write more than DUMP_LIMIT_BYTES in all."""
    import numpy as np
    total = sum(a.nbytes for _, a in arrays)
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES} byte limit")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays:
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(path, name + ".npy"), a)


def step_outputs(logs, nets):
    """What a caller of the train step receives from its last call: the losses (float64 scalars, `loss_<key>`) and the networks'
    state after it (`<net>.<state_dict key>`, float32, sampled by dump_sample)."""
    import numpy as np
    out = [(f"loss_{k}", np.asarray(float(v), dtype=np.float64)) for k, v in logs.items()]
    for tag, net in nets:
        if net is not None:
            out += [(f"{tag}.{k}", dump_sample(v, f"{tag}.{k}")) for k, v in net.state_dict().items() if v.is_floating_point()]
    return out


def snapshot_state(G, D, vgg):
    """CPU copies of the three state dicts (taken BEFORE the first GPU step, for the oracle's parity step)."""
    f = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()} if m is not None else None
    return f(G), f(D), f(vgg)


def cpu_baseline(args, state, batch):
    """The same train step on the host cores through the CPU oracle (oracle/step.py): 1 warm-up + 3 timed steps
    (BASELINE.md section 3), best and median.  The warm-up step starts from the weights and the batch of GPU step 0, so
    its losses double as the parity check of the benchmarked configuration.  Also: BASELINE config 1 (G inference
    [1,3,48,48] -> [1,3,192,192] on the CPU), 1 warm-up + 5 timed.  -> (cpu_baseline dict, losses of the parity step)"""
    import statistics
    from oracle import model as OM
    from oracle import step as OS
    nthreads = host_cores()
    torch.set_num_threads(nthreads)
    g_sd, d_sd, v_sd = state
    lr, hr = batch
    B = lr.size(0)
    cfg = {"depth": args.num_blocks, "res_scale": 0.1, "learning_rate": args.lr}
    st = OS.TrainState(g_sd, d_sd, v_sd, cfg)
    step = OS.gan_step if args.workload == "gan" else OS.pretrain_step
    from oracle import bf16 as OB
    with OB.enabled(args.precision == "bf16"):     # (bf16 row: the parity step restates the bf16 mode; the timed steps below are
        first = step(st, lr, hr)                   #  the reference's fp32 arithmetic either way)  warm-up = parity step
        first = {k: float(v) for k, v in first.items()}
        if args.precision == "bf16":
            # The bf16 mode's own noise floor at this configuration: a difference of one fp32 ulp upstream can flip a bf16 rounding
            # downstream (2^-8 of that operand), so two exact-arithmetic-equivalent evaluations differ by far more than fp32
            # rounding.  Measured, not assumed: the same step with every weight moved one ulp up / one ulp down.
            floor = 0.0
            for direction in (float("inf"), -float("inf")):
                mv = lambda sd: {k: (torch.nextafter(v, torch.full_like(v, direction)) if v.is_floating_point() else v.clone())
                                 for k, v in sd.items()}
                alt = step(OS.TrainState(mv(g_sd), mv(d_sd) if d_sd else None, v_sd, cfg), lr, hr)
                floor = max([floor] + [abs(float(alt[k]) - first[k]) / max(abs(first[k]), 1e-12) for k in first])
            first["_noise_floor"] = floor
    times = []
    for _ in range(args.cpu_steps):
        t0 = time.perf_counter()
        step(st, lr, hr)
        times.append(time.perf_counter() - t0)
    best, med = min(times), statistics.median(times)
    x1 = lr[:1]
    with torch.no_grad():
        OM.generator_forward(g_sd, x1, args.num_blocks, 0.1)
        t1 = []
        for _ in range(5):
            t0 = time.perf_counter()
            OM.generator_forward(g_sd, x1, args.num_blocks, 0.1)
            t1.append(time.perf_counter() - t0)
    try:
        cpu_model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        cpu_model = "unknown"
    return {"value": B / best, "unit": "patches/s", "cores": nthreads, "kind": "port", "median": B / med,
            "step_s_best": round(best, 3), "step_s_median": round(med, 3), "cpu_model": cpu_model,
            "sample": f"{args.cpu_steps} timed {args.workload} steps (after 1 warm-up) of the CPU oracle (torch {torch.__version__} "
                      f"CPU ops) at batch {B}, full model size; value = best, median alongside",
            "config1_infer": {"workload": "BASELINE config 1: G forward no_grad [1,3,48,48] -> [1,3,192,192], CPU oracle",
                              "s_best": round(min(t1), 4), "s_median": round(statistics.median(t1), 4),
                              "images_per_s": round(1.0 / min(t1), 3)}}, first


def bench_infer512(args, device):
    """BASELINE config 5 (side measurement, 1 GPU): G forward, no_grad, 4 x 512x512 LR -> 2048x2048; 105.39 TFLOP per batch."""
    from model import Generator
    torch.manual_seed(0)
    G = Generator({"num_channels": 256, "depth": 32, "res_scale": 0.1}).to(device)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (4, 3, 512, 512), generator=g).float().to(device)
    with torch.no_grad():
        for _ in range(max(1, args.warmup)):
            G(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = G(x)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, [("sr", dump_sample(y, "sr", 1 << 22))])
    tf = 105.3875 / dt
    bf16 = args.precision == "bf16"
    peak = PEAK_BF16_MFMA_TFLOPS if bf16 else PEAK_F32_MFMA_TFLOPS
    print(json.dumps({"metric": "LR tiles/sec (x4 SR generator forward, 512x512 LR tiles, batch 4)" + (" [OPTIONAL bf16-operand mode]" if bf16 else ""),
                      "value": round(4 / dt, 3),
                      "unit": "tiles/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 2),
                      "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                      "dtype": "bf16 operands / f32 accumulation in the 3x3 convs, f32 tensors" if bf16 else "f32", "data": "synthetic",
                      "precision": args.precision,
                      "config": {"workload": "BASELINE config 5: G forward no_grad, 4x3x512x512 -> 4x3x2048x2048, 256 ch x 32 blocks"},
                      "step_tflops_per_gpu": round(tf, 2), "step_frac_of_mfma_peak": round(tf / peak, 4), "mfma_peak_tflops": peak,
                      "out_checksum": float(y.double().sum())}), flush=True)


def main():
    if os.environ.get("PESR_DUMP_STACKS_AFTER"):       # debugging aid for a hung multi-rank run: every thread's Python stack to stderr after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["PESR_DUMP_STACKS_AFTER"]), exit=False)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["gan", "pretrain", "infer512"], default="gan",
                    help="gan = BASELINE config 3/4 (the headline metric); pretrain = config 2; infer512 = config 5 "
                         "(G forward on 4 x 512x512 LR tiles, no_grad) - the latter two are side measurements")
    ap.add_argument("--batch", type=int, default=16, help="per-GPU batch")
    ap.add_argument("--patch_size", type=int, default=48)
    ap.add_argument("--num_channels", type=int, default=256)
    ap.add_argument("--num_blocks", type=int, default=32)
    ap.add_argument("--cpu_steps", type=int, default=3, help="timed CPU-oracle steps (after one warm-up / parity step)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU oracle (cpu_baseline and parity_check)")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--event-every", type=int, default=8,
                    help="bracket every n-th launch of each watched kernel kind with HIP events (all ~200 per step cost 2 %% of the step)")
    ap.add_argument("--hip-graph", action="store_true",
                    help="capture the step into a hipGraph after the warm-up and time replays (bit-identical results; with N > 1 the "
                         "RCCL all-reduces are captured with it; the roofline kernel events are then taken from two extra eager steps "
                         "outside the timed region)")
    ap.add_argument("--precision", choices=["fp32", "bf16", "split-bf16"], default="fp32",
                    help="fp32 (default, the headline): the reference's arithmetic.  bf16: the OPTIONAL bf16-operand mode (SURVEY 8 f4) - "
                         "a separate row with its own oracle, tolerance and 2.5 PFLOP/s roofline denominator.  split-bf16: the OPTIONAL "
                         "split mode (three bf16 products per multiply, 4e-6 of the output maximum): a separate row too, checked against "
                         "the fp32 oracle at the fp32 tolerance")
    ap.add_argument("--dp-policy", choices=["auto", "overlap", "defer_g", "defer_all"], default="auto",
                    help="data-parallel schedule (N > 1, or PESR_FORCE_DP=1): auto = measured inside the warm-up - 3 steps each of "
                         "eager overlap / G's all-reduce deferred behind its backward pass / both deferred, then the captured hipGraph "
                         "step with the best of them - and the timed region runs the fastest (Trainer.calibrate_dp_policy)")
    ap.add_argument("--calib-steps", type=int, default=3, help="timed steps per candidate of --dp-policy auto")
    ap.add_argument("--no-graph-candidate", action="store_true", help="--dp-policy auto: eager candidates only")
    ap.add_argument("--no-peer-candidate", action="store_true",
                    help="N > 1: do not time the CU-free gradient exchange over peer memory (comm.PeerCopy: IPC mappings, stream wait / "
                         "write-value operations, peer copies; rehearsed in child processes first) as a candidate of --dp-policy auto")
    ap.add_argument("--no-side", action="store_true",
                    help="skip the side measurements of BASELINE configs 2 and 5 (pretrain step, G forward on 4 x 512x512 LR tiles) that a "
                         "1-GPU run of the default workload appends to its JSON line")
    ap.add_argument("--batches", type=int, default=4, help="distinct synthetic batches rotated through the steps")
    ap.add_argument("--lr", type=float, default=5e-7,
                    help="Adam learning rate of both optimizers.  The reference's 5e-5 (SURVEY 8d) lets the Discriminator separate "
                         "white-noise HR crops from an untrained Generator's output within ~15 steps: its loss falls to 1e-15 and its "
                         "backward pass then runs on zeros, whatever the batch (measured with 4 rotating batches).  The work of a step "
                         "does not depend on the value, so the default keeps the losses O(0.1 .. 1) for the whole run instead")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the CPU oracle (cpu_baseline, parity_check), the side measurements, "
                         "roofline kernel events, the matrix-pipe tally, host enqueue time and, with N > 1, per-collective and exposed-"
                         "communication timing, the peer-copy engine probe and the replica check.  Off: set up, warm up, time the steps")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (rank 0): the losses and the "
                         "networks' state after it, tensors above %d elements as a fixed, seeded sample" % DUMP_SAMPLE)
    args = ap.parse_args()

    under_launcher = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if args.gpus > 1 and not under_launcher:
        self_launch(args)                         # never returns
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # TEST HOOK (tests/test_dp_gpu.py): PESR_DP_SHARE_GPU=1 + PESR_DP_BACKEND=gloo lets N ranks time-share cuda:0 over gloo, so that
    # every world > 1 branch of this script runs on a one-GPU box.  Not a measurement mode: the JSON says so (`test_hook`).
    share_gpu = os.environ.get("PESR_DP_SHARE_GPU") == "1"
    backend = os.environ.get("PESR_DP_BACKEND", "nccl")
    if share_gpu:
        assert backend == "gloo", "RCCL refuses two ranks on one device"
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    n_seen = 1
    if under_launcher:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)                     # the GPU count RCCL really spans
        n_seen = int(ones.item())
        if n_seen != args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: the RCCL group spans {n_seen} rank(s)")

    from pesr_amd import ops
    ops.set_precision(args.precision)
    if args.workload == "infer512":
        return bench_infer512(args, device)
    trainer, G, D, vgg = build(args, device, world)
    # NBATCH distinct synthetic batches, rotated: with ONE fixed batch the Discriminator separates it within ~20 steps, its loss
    # falls to 1e-7 and D's backward pass then runs on near-zero data (never time kernels on zeros)
    batches = [synth_batch(args.batch, args.patch_size, 1234 + rank + 1000 * i, device) for i in range(max(1, args.batches))]
    lr, hr = batches[0]
    eager_step = trainer.gan_step if args.workload == "gan" else trainer.pretrain_step
    step = eager_step
    full = args.full
    want_cpu = full and not args.no_cpu_baseline and world == 1
    state0 = snapshot_state(G, D, vgg) if want_cpu else None
    nstep = [0]

    def next_batch():
        b = batches[nstep[0] % len(batches)]
        nstep[0] += 1
        return b

    def run(fn):
        return fn(*next_batch())

    # step 0 (always eager, on batch 0): its losses go to the parity check as host floats, and (--full) the matrix-pipe work of
    # one step is tallied while it runs
    if full:
        ops.FLOPS.start()
    first_log = {k: float(v) for k, v in run(eager_step).items()}
    flops = ops.FLOPS.stop() if full else None
    use_graph = args.hip_graph and args.workload in ("gan", "pretrain")
    optims = [o for o in (trainer.optim_D, trainer.optim_G) if o is not None]
    dp_on = all(o.buckets.enabled for o in optims)      # world > 1, or PESR_FORCE_DP=1 over a one-rank group
    for _ in range(max(args.warmup, 2 if (use_graph or dp_on) else 0) - 1):     # (a capture needs two eager steps behind it)
        run(eager_step)
    torch.cuda.synchronize()
    watch = (args.batch, args.patch_size, args.patch_size, args.num_channels, args.num_channels, 1)
    dp_info = None
    if dp_on and not use_graph:
        # The data-parallel schedule is chosen by measurement, still inside the warm-up (untimed; real optimizer steps)
        if args.dp_policy == "auto":
            dp_info = trainer.calibrate_dp_policy(args.workload, next_batch, steps=args.calib_steps, graph=not args.no_graph_candidate,
                                                  peer_candidate=not args.no_peer_candidate)
            step = trainer.dp_step
            use_graph = dp_info["chosen"].startswith("graph")
        else:
            trainer.set_dp_policy(args.dp_policy)
            dp_info = {"chosen": args.dp_policy, "forced": True, "transport": trainer._transports()[0].name}
            run(eager_step)
        torch.cuda.synchronize()
    elif dp_on:
        if args.dp_policy != "auto":
            trainer.set_dp_policy(args.dp_policy)
            run(eager_step); run(eager_step)
        dp_info = {"chosen": "graph+" + trainer.dp_policy, "forced": True, "transport": trainer._transports()[0].name}
    if use_graph and step is eager_step:
        step = trainer.capture_gan_step(lr, hr) if args.workload == "gan" else trainer.capture_pretrain_step(lr, hr)
        run(step)                                   # first replay outside the timed region (graph upload)
        torch.cuda.synchronize()
    if full and not use_graph and not args.no_kernel_events:
        ops.KERNEL_EVENTS.enable(shape=watch, every=args.event_every)
    for o in optims:
        o.buckets.measure_exposed = full and not use_graph
    dp_transports = trainer._transports() if dp_on else []
    for t_ in dp_transports:
        t_.collective_times()                      # (drop whatever the warm-up left)
        t_.time_collectives = full and not use_graph    # HIP events on the communication stream around every all-reduce of the timed steps
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        logs = run(step)
    host_done = time.perf_counter() - t0            # the host has enqueued all K steps; the GPU is (normally) still running
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = my_elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:    # before anything below runs another step on these networks
        dump_outputs(args.dump_outputs, step_outputs(logs, (("G", G), ("D", D))))
    exposed = [o.buckets.exposed_ms() for o in optims]
    for o in optims:
        o.buckets.measure_exposed = False
    coll = []
    for t_ in dp_transports:
        t_.time_collectives = False
        coll += t_.collective_times()
    # which engine moved the peer copies (only the peer-memory transport has any), and: are the replicas still identical?
    peer_engine = None
    if full and dp_transports and dp_transports[0].name == "peer-copy" and world > 1:
        peer_engine = dp_transports[0].copy_engine_probe(optims[-1].flat.flat_g)
    replica_check = None
    if full and world > 1:
        sums = torch.stack([o.flat.flat_p.double().sum() for o in optims] + [o.flat.flat_p.double().abs().sum() for o in optims])
        lo, hi = sums.clone(), sums.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replica_check = {"identical": bool(torch.equal(lo, hi)), "what": "sum and abs-sum (float64) of every optimizer's flat parameter buffer after the "
                         "timed steps: MIN over ranks == MAX over ranks (replicas that received different gradient sums diverge)"}
    if full and use_graph and not args.no_kernel_events:     # events cannot be read back from inside a graph: two eager steps for them
        ops.KERNEL_EVENTS.enable(shape=watch)
        for _ in range(2):
            run(eager_step)
    kern = ops.KERNEL_EVENTS.drain()
    host_enqueue_ms = None
    if full:
        # host cost of ONE eager step: enqueue three steps on an idle GPU without waiting for it (python + launches only)
        torch.cuda.synchronize()
        th = time.perf_counter()
        for _ in range(3):
            run(eager_step)
        host_enqueue_ms = 1e3 * (time.perf_counter() - th) / 3
        torch.cuda.synchronize()
    per_rank = None
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        per_rank = [float(g.item()) for g in gathered]
        elapsed = max(per_rank)
        if full:
            hh = torch.tensor([host_enqueue_ms, host_done], device=device, dtype=torch.float64)
            dist.all_reduce(hh, op=dist.ReduceOp.MAX)
            host_enqueue_ms, host_done = float(hh[0]), float(hh[1])
    if rank != 0:
        from pesr_amd import comm
        comm.close_transports()
        dist.destroy_process_group()
        return

    global_batch = args.batch * world
    value = args.steps * global_batch / elapsed
    flop_patch = GFLOP_PER_PATCH[args.workload] * 1e9
    bf16 = args.precision == "bf16"
    split = args.precision == "split-bf16"
    peak = PEAK_BF16_MFMA_TFLOPS if (bf16 or split) else PEAK_F32_MFMA_TFLOPS
    out = {
        "metric": "HR-patches/sec (x4 SR GAN train step, 48->192)" + (" [OPTIONAL bf16-operand mode, not the headline]" if bf16 else
                                                                      " [OPTIONAL split-bf16 mode, not the headline]" if split else ""),
        "value": round(value, 3), "unit": "patches/s", "n_gpus": n_seen, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "data": "synthetic",
        "dtype": ("bf16 operands / f32 accumulation in the 3x3 convs the bf16 kernels cover (G body, upsamplers, the larger D / VGG layers); "
                  "f32 tensors, optimizer and every other op") if bf16 else
                 ("f32 operands split into hi + lo bf16 terms, three bf16 MFMA products per multiply, f32 accumulation, in the forward / "
                  "input gradient of the stride-1 convs with Cout % 128 == 0; f32 kernels for weight gradients and every other op") if split else "f32",
        "precision": args.precision,
        "config": {"workload": ("full GAN phase (G + D + VGG + RSGAN focal loss), " if args.workload == "gan"
                                else "pretrain phase (L1 only), ") +
                               f"per-GPU batch {args.batch}, LR {args.patch_size}x{args.patch_size} -> HR "
                               f"{4 * args.patch_size}x{4 * args.patch_size}, {args.num_channels} ch x {args.num_blocks} blocks" +
                               (f"; Adam lr {args.lr:g} instead of the reference's 5e-5 (same work per step; keeps D's loss O(0.1) on "
                                "white-noise crops, see `lr_note`)" if args.lr != 5e-5 else ""),
                   "global_batch": global_batch, "parallelism": f"dp{world}"},
        "step_tflops_per_gpu": round(value / world * flop_patch / 1e12, 2),
        # ALGORITHMIC flops / time / peak: may exceed 1 because the Winograd kernels issue 1/2 .. 2/3 of them
        "step_frac_of_mfma_peak": round(value / world * flop_patch / (peak * 1e12), 4),
        "mfma_peak_tflops": peak,
        "losses": {k: float(v) for k, v in logs.items()},
        "losses_step0": first_log,
        "batches_rotated": len(batches), "lr": args.lr,
        "lr_note": ("DEVIATION from SURVEY 8d's --learning_rate 5e-5: at 5e-5 the Discriminator separates white-noise HR crops from an "
                    "untrained Generator within ~15 steps, its loss falls to 1e-15 and its backward pass runs on zeros (never time kernels "
                    "on zeros); the work of a step does not depend on the value.  `--lr 5e-5` reproduces the reference's flag (same box, "
                    "same build: 216.2 vs 216.9 patches/s, DESIGN.md 6)") if args.lr != 5e-5 else None,
        "hip_graph": bool(use_graph),
        "force_dp": os.environ.get("PESR_FORCE_DP") == "1",
        "full": full,
    }
    if full:
        out.update({
            # flops the step's kernels really ISSUE on the matrix pipe (tallied per launch during step 0) / time / peak: the honest
            # whole-step hardware fraction
            "step_issued_frac": round(flops["issued"] / (1e3 * elapsed / args.steps) / 1e9 / peak, 4),
            "step_flops": {"algorithmic_tflop_counted": round(flops["algorithmic"] / 1e12, 3), "issued_tflop": round(flops["issued"] / 1e12, 3),
                           "by_kernel_family_tflop": {k: [round(a / 1e12, 3), round(b / 1e12, 3)] for k, (a, b) in flops["by_kernel_family"].items()},
                           "note": "per family: [algorithmic, issued on the matrix pipe]; counted from the launches of step 0"},
            # host side: time to ENQUEUE one eager step (python + launches, GPU idle at start, no waiting) and the moment the host
            # had enqueued all K timed steps relative to their completion (max over ranks)
            "host_enqueue_ms": round(host_enqueue_ms, 2),
            "host_enqueue_frac_of_step": round(host_enqueue_ms / (1e3 * elapsed / args.steps), 3),
            "host_done_ms_before_gpu": round(1e3 * (my_elapsed - host_done), 1),
        })
    if share_gpu:
        out["test_hook"] = f"{world} ranks time-sharing cuda:0 over {backend}: exercises the multi-rank code path, NOT a measurement"
    if dp_info is not None:
        out["dp_policy"] = dp_info
        out["dp_policy_note"] = ("data-parallel schedule measured inside the warm-up (ms per step, max over ranks): overlap = bucketed "
                                 "all-reduces launched from the autograd hooks under backward; defer_g = G's gradients as ONE all-reduce after "
                                 "its backward pass; defer_all = D's too; graph+X = the step with schedule X captured as one hipGraph; the timed "
                                 "region ran `chosen`")
    if dp_info is not None and dp_on:
        from pesr_amd import comm as _comm
        out["dp_bringup"] = _comm.bringup_log()
        out["dp_transport"] = {"name": dp_transports[0].name if dp_transports else None,
                               "fallback_reason": dp_info.get("fallback_reason") or getattr(dp_transports[0], "fallback_reason", None) if dp_transports else None}
    if coll:
        # per bucket size: mean time on the communication stream (from the collective's start - which includes waiting for the slowest
        # peer to arrive - to its end) and the rates that follow: algbw = bytes / time, busbw = algbw x 2 (N - 1) / N (ring convention)
        by = {}
        for nb, ms_ in coll:
            by.setdefault(nb, []).append(ms_)
        fac = 2.0 * (world - 1) / world if world > 1 else 1.0
        out["dp_collectives"] = {"per_step": round(len(coll) / args.steps, 2),
                                 "buckets": [{"bytes": nb, "n": len(v), "mean_ms": round(sum(v) / len(v), 3), "min_ms": round(min(v), 3),
                                              "algbw_GB_per_s": round(nb / (sum(v) / len(v)) / 1e6, 1), "busbw_GB_per_s": round(fac * nb / (sum(v) / len(v)) / 1e6, 1),
                                              "busbw_best_GB_per_s": round(fac * nb / min(v) / 1e6, 1)} for nb, v in sorted(by.items())],
                                 "total_ms_per_step": round(sum(m for _, m in coll) / args.steps, 3),
                                 "note": "rank 0, HIP events on the transport's communication stream around every gradient all-reduce of the timed steps; "
                                         "the time includes waiting for the last rank to reach the collective and any slowdown from sharing the GPU with backward kernels"}
    if peer_engine is not None:
        out["peer_copy_engine"] = peer_engine
    if replica_check is not None:
        out["replica_check"] = replica_check
    if any(n for _, n in exposed):
        out["comm_exposed_ms"] = round(sum(ms for ms, n in exposed if n), 3)
        out["comm_exposed_ms_by_optimizer"] = {("D" if o is trainer.optim_D else "G"): round(ms, 3) for o, (ms, n) in zip(optims, exposed) if n}
        out["comm_exposed_note"] = ("per step: time the compute stream stood waiting in FlatAdam.step for gradient all-reduces that "
                                    "backward had not covered (HIP events around the waits, D + G optimizers, rank 0)")
    if per_rank:
        out["per_rank_ms_per_step"] = {"min": round(1e3 * min(per_rank) / args.steps, 3), "max": round(1e3 * max(per_rank) / args.steps, 3)}
    if kern:
        out.update(roofline_objects(args, kern))
    if want_cpu:
        out["cpu_baseline"], ref0 = cpu_baseline(args, state0, (batches[0][0].cpu(), batches[0][1].cpu()))
        got0 = first_log
        floor = ref0.pop("_noise_floor", None)
        rel = {k: abs(got0[k] - ref0[k]) / max(abs(ref0[k]), 1e-12) for k in ref0 if abs(ref0[k]) > 0 or abs(got0[k]) > 0}
        worst = max(rel.values()) if rel else 0.0
        # bf16 row: against the oracle's restatement of the bf16 mode (oracle/bf16.py), to 5e-4 or three times the mode's MEASURED
        # noise floor at this configuration (the oracle's own losses with every weight moved by one fp32 ulp), whichever is larger
        # ... capped at 5e-3: an ill-conditioned configuration must not widen its own tolerance without bound - if three floors
        # exceed the cap the check is reported as inconclusive, not as passed
        BF16_TOL_CAP = 5e-3
        ptol = min(max(5e-4, 3.0 * floor), BF16_TOL_CAP) if bf16 else 5e-5
        inconclusive = bool(bf16 and 3.0 * floor > BF16_TOL_CAP)
        out["parity_check"] = {"what": "losses of GPU step 0 vs the CPU oracle's step from the same initial weights and batch "
                                       "(benchmarked configuration and kernel dispatch)",
                               "max_rel_loss_err": worst, "tol": ptol, "ok": bool(worst <= ptol) and not inconclusive,
                               "gpu": got0, "cpu_oracle": ref0}
        if floor is not None:
            out["parity_check"]["oracle_one_ulp_noise_floor"] = floor
            if inconclusive:
                out["parity_check"]["verdict"] = f"inconclusive: 3 x the oracle's own one-ulp noise floor exceeds the cap {BF16_TOL_CAP}"
    if full and args.workload == "gan" and world == 1 and not args.no_side and not bf16 and not split:
        out["side"] = side_measurements(args, trainer, G, batches, device)
    print(json.dumps(out), flush=True)
    if dist.is_initialized():
        from pesr_amd import comm
        comm.close_transports()
        dist.destroy_process_group()


def side_measurements(args, trainer, G, batches, device):
    """BASELINE configs 2 and 5 inside the driver's one default run (1 GPU, after the timed GAN region; side figures, never
    `value`): the pretrain step on the same Generator and batches (5 timed steps), and the Generator forward on 4 x 512x512 LR
    tiles (3 timed batches) with HIP-event times of its HBM-bound layers (upsample.4, embed, MeanShift vs 6.29 TB/s
    measured / 8 TB/s spec; algorithmic bytes = SURVEY Appendix A.4 "min MB")."""
    from pesr_amd import ops
    side = {}
    # ---- the reference's own --learning_rate 5e-5 (reference train.py:46), from the INITIAL weights -----------------
    # The timed region runs at --lr (default 5e-7, `lr_note`).  Same seeds, a second set of networks, Adam at 5e-5: two untimed
    # and five timed GAN steps, the Discriminator's loss after every one of them in the record (on white-noise crops it separates real
    # from generated within a handful of steps at this rate - which is why the timed region does not use it), so that the two rates
    # can be compared in one driver-attested line.
    if args.workload == "gan" and abs(args.lr - 5e-5) > 1e-12:
        import copy
        a2 = copy.copy(args)
        a2.lr = 5e-5
        tr2, G2, D2, V2 = build(a2, device, 1)
        d_trace = []
        for i in range(2):
            d_trace.append(tr2.gan_step(*batches[i % len(batches)])["d"])
        torch.cuda.synchronize()
        n = 5
        t0 = time.perf_counter()
        for i in range(n):
            log2 = tr2.gan_step(*batches[(2 + i) % len(batches)])
            d_trace.append(log2["d"])
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / n
        side["lr_5e-5"] = {"workload": "the timed workload at the reference's --learning_rate 5e-5 (reference train.py:46), from the initial "
                                       "weights: 2 untimed + 5 timed eager GAN steps",
                           "steps": n, "ms_per_step": round(ms, 3), "patches_per_s": round(args.batch / ms * 1e3, 2),
                           "losses_after": {k: float(v) for k, v in log2.items()},
                           "d_loss_per_step": [float(v) for v in d_trace],      # (the 2 untimed steps, then the 5 timed ones: shows when D separates the noise crops)
                           "note": "compare with the line's own ms_per_step (Adam at %g): the work of a step does not depend on the value "
                                   "of the learning rate" % args.lr}
        del tr2, G2, D2, V2, log2
        torch.cuda.empty_cache()
    # ---- config 2: pretrain step (reference train.py:164-173) -----------------------------------------------------------
    for b in batches[:2]:
        trainer.pretrain_step(*b)
    ops.FLOPS.start()
    trainer.pretrain_step(*batches[0])
    fl = ops.FLOPS.stop()
    torch.cuda.synchronize()
    n = 5
    t0 = time.perf_counter()
    for i in range(n):
        trainer.pretrain_step(*batches[i % len(batches)])
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / n
    pps = args.batch / ms * 1e3
    side["pretrain"] = {"workload": f"BASELINE config 2: pretrain phase (L1 only), batch {args.batch}, LR {args.patch_size}x{args.patch_size}, "
                                    f"{args.num_channels} ch x {args.num_blocks} blocks, eager",
                        "steps": n, "ms_per_step": round(ms, 3), "patches_per_s": round(pps, 2),
                        "algorithmic_frac_of_mfma_peak": round(pps * GFLOP_PER_PATCH["pretrain"] * 1e9 / (PEAK_F32_MFMA_TFLOPS * 1e12), 4),
                        "issued_frac_of_mfma_peak": round(fl["issued"] / ms / 1e9 / PEAK_F32_MFMA_TFLOPS, 4),
                        "issued_tflop_per_step": round(fl["issued"] / 1e12, 3)}
    # ---- config 5: G forward, no_grad, 4 x 512x512 LR -> 2048x2048 (105.39 TFLOP per batch) ------------------------------
    trainer.optim_G.zero_grad()
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (4, 3, 512, 512), generator=g).float().to(device)
    with torch.no_grad():
        G(x)                                                  # warm-up: packings for this shape, allocator growth
        ops.FLOPS.start()
        G(x)
        fl5 = ops.FLOPS.stop()
        torch.cuda.synchronize()
        ops.OP_EVENTS.enable()
        n5 = 3
        t0 = time.perf_counter()
        for _ in range(n5):
            y = G(x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n5
    ev = ops.OP_EVENTS.drain()
    del y
    torch.cuda.empty_cache()
    # algorithmic HBM bytes (each layer reads its input once, writes its output once, reads its weights once)
    px_lr, px_hr = 4 * 512 * 512, 4 * 2048 * 2048
    alg = {"conv_rgb_out 256->3": (px_hr * (256 + 3) * 4 + 3 * 256 * 9 * 4, "upsample.4 (256->3 @2048x2048)"),
           "conv_rgb_in 3->256": (px_lr * (3 + 256) * 4 + 256 * 27 * 4, "embed (3->256 @512x512)"),
           "meanshift 512x512": (px_lr * 6 * 4, "sub_mean (1x1, 3->3 @512x512)"),
           "meanshift 2048x2048": (px_hr * 6 * 4, "add_mean (1x1, 3->3 @2048x2048)")}
    hbm = {}
    for k, (msk, nk) in ev.items():
        if k in alg:
            by, label = alg[k]
            hbm[label] = {"avg_us": round(msk * 1e3, 1), "launches_timed": nk, "algorithmic_MB": round(by / 1e6, 1),
                          "GB_per_s": round(by / (msk * 1e-3) / 1e9, 1), "frac_of_6.29TBps_measured": round(by / (msk * 1e-3) / 6.29e12, 3),
                          "frac_of_8TBps_spec": round(by / (msk * 1e-3) / 8e12, 3)}
    tf = 105.3875 / dt
    side["infer512"] = {"workload": "BASELINE config 5: G forward no_grad, 4x3x512x512 -> 4x3x2048x2048, 256 ch x 32 blocks",
                        "batches": n5, "ms_per_batch": round(dt * 1e3, 2), "tiles_per_s": round(4 / dt, 3),
                        "algorithmic_tflops": round(tf, 2), "algorithmic_frac_of_mfma_peak": round(tf / PEAK_F32_MFMA_TFLOPS, 4),
                        "issued_frac_of_mfma_peak": round(fl5["issued"] / dt / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                        "hbm_bound_kernels": hbm,
                        "hbm_note": "HIP events on the launch stream around every launch of these ops inside the timed batches; bytes are "
                                    "ALGORITHMIC (SURVEY Appendix A.4 'min MB'), PMC traffic for the same kernels: profiles/r06_hbm_pmc_summary.csv, request counters profiles/r06_hbm_tcc_summary.csv"}
    return side


def roofline_objects(args, kern):
    """`roofline` (the dominant kernel: forward of the G body conv) + `roofline_kernels` (the other two body kernels).
    achieved = ALGORITHMIC flops of the conv / mean HIP-event duration of its launches inside the timed steps;
    frac = flops the kernel ISSUES on the matrix pipe (1/2 of the algorithmic ones for the 1-D Winograd F(4,3) kernels, 2/3 for F(2,3),
    1/3 for the weight gradient's y-nested form)
    / duration / peak, i.e. matrix-pipe utilisation - the honest hardware fraction; algorithmic_frac = achieved / peak."""
    from pesr_amd import ops as _ops
    scale = (args.batch / 16) * (args.patch_size / 48) ** 2 * (args.num_channels / 256) ** 2
    bs = (args.batch, args.patch_size, args.patch_size, args.num_channels, args.num_channels)
    # (kernel name, fraction of the conv's algorithmic flops the kernel issues on the matrix pipe)
    bf16 = getattr(args, "precision", "fp32") in ("bf16", "split-bf16")
    peak = PEAK_BF16_MFMA_TFLOPS if bf16 else PEAK_F32_MFMA_TFLOPS
    if _ops.bf16x3_eligible(*bs):
        conv_k = ("conv3x3_bf16x3_kernel", 3.0)
    elif _ops.bf16_eligible(*bs):
        conv_k = ("conv3x3_bf16_kernel", 1.0)
    elif _ops.wino4_eligible(*bs):
        conv_k = ("conv3x3_wino4_kernel", 0.5)
    elif _ops.wino_eligible(*bs):
        conv_k = ("conv3x3_wino_kernel", 2.0 / 3.0)
    else:
        conv_k = ("conv3x3_mfma_kernel<1, 8, 9, 2, 1, 2", 1.0)
    wg_wino = _ops.USE_WGRAD_WINO and args.patch_size % 2 == 0 and args.patch_size >= 48 and args.num_channels % 64 == 0
    wg_k = _ops.wgrad_kernel_for(*bs) if hasattr(_ops, "wgrad_kernel_for") else \
        (("conv3x3_wgrad_wino_kernel", 2.0 / 3.0) if wg_wino else ("conv3x3_wgrad_kernel", 1.0))
    if _ops.wgrad_bf16_eligible(*bs):
        wg_k = ("conv3x3_wgrad_bf16_kernel", 1.0)
    shape = f"G body {args.num_channels}->{args.num_channels} @{args.patch_size}x{args.patch_size}, batch {args.batch}"
    names = {"fwd": conv_k + (f"forward ({shape}: 65 G launches + the 6 same-shaped VGG conv3_2..3_4 launches per GAN step)",),
             "dgrad": conv_k + (f"input gradient ({shape}: 65 G + 3 VGG launches per GAN step)",),
             "wgrad": wg_k + (f"weight gradient incl. its split-K reduce kernel ({shape}: 65 launches per step)",)}
    objs = {}
    for kind, (ms, n) in kern.items():
        kname, issue_frac, label = names[kind]
        ach = K1_GFLOP * scale / ms                                  # algorithmic TFLOP/s
        issued = ach * issue_frac
        traffic, src, stamp = k1_hbm_traffic_bytes(kname)
        o = {"kernel": f"{kname} {label}", "bound": "mfma", "achieved": round(ach, 2), "peak": peak,
             "unit": "TFLOP/s", "frac": round(issued / peak, 4),
             "algorithmic_frac": round(ach / peak, 4), "issued_tflops": round(issued, 2),
             "traffic": traffic,
             "traffic_note": (f"HBM bytes/launch (2*FETCH_SIZE + WRITE_SIZE) from the separate rocprofv3 --pmc passes in profiles/{src}"
                              if src else stamp),
             "traffic_source_commit": (f"sha256[:16] of pesr_amd/csrc/{KERNEL_SOURCE.get(kname.split('<')[0].strip())} the counters were "
                                       f"taken on = {stamp} (matches the source this run was built from)") if src else None,
             "launches_timed": n, "avg_launch_us": round(ms * 1e3, 2),
             "sampling": ("every launch of this kind in two eager steps after the timed graph replays is bracketed by HIP events"
                          if getattr(args, "hip_graph", False) else
                          f"every {getattr(args, 'event_every', 1)}-th launch of this kind inside the timed steps is bracketed by HIP events")}
        if issue_frac > 1.0 and kname == "conv3x3_bf16x3_kernel":
            o["peak"] = PEAK_BF16_MFMA_TFLOPS
            o["frac"] = round(issued / PEAK_BF16_MFMA_TFLOPS, 4)
            o["algorithmic_frac"] = round(ach / PEAK_BF16_MFMA_TFLOPS, 4)
            o["note"] = ("split-bf16: three v_mfma_f32_16x16x32_bf16 products per multiply; frac = issued bf16 flops (3 x algorithmic) / "
                         "duration / the nominal 2.5 PFLOP/s")
        elif kind == "wgrad" and bf16 and kname != "conv3x3_wgrad_bf16_kernel":
            o["peak"] = PEAK_F32_MFMA_TFLOPS        # the weight gradient of this row stays on the fp32 kernels
            o["frac"] = round(issued / PEAK_F32_MFMA_TFLOPS, 4)
            o["algorithmic_frac"] = round(ach / PEAK_F32_MFMA_TFLOPS, 4)
        if issue_frac < 1.0:
            form, part = (("1-D Winograd F(4,3)", "1/2") if issue_frac == 0.5 else
                          ("Winograd F(4,3) along x nested with F(2,3) along y", "1/3") if issue_frac < 0.4 else ("1-D Winograd F(2,3)", "2/3"))
            o["note"] = (f"{form}: the kernel issues {part} of the direct conv's MFMA flops; frac counts the ISSUED flops "
                         "(matrix-pipe utilisation), algorithmic_frac the conv's algorithmic flops")
        objs[kind] = o
    out = {}
    if "fwd" in objs:
        out["roofline"] = objs.pop("fwd")
    if objs:
        out["roofline_kernels"] = [objs[k] for k in ("dgrad", "wgrad") if k in objs]
    return out


if __name__ == "__main__":
    main()
