"""Where the F(4,3) forward / input-gradient kernel's time goes at the G-body shape ([16,48,48,256] -> 256), per phase and per ablation,
and the A/B of its two loops: the chunk loop (PESR_WINO4_TAIL=0) and the same loop with the TAIL form of its last chunk
(docs/experiments/wino4_loop.md, wino4_tail.md; the loop before them was retired: docs/experiments/wino4_retire.md).

    python scripts/wino4_loop.py build            # no GPU needed: conv3x3_wino4.hip once per variant (-DW4_STAMPS, -DW4_NO_*), each linked
                                                  # with the objects of the regular build into a library of its own, exp/libw4_<variant>.so
    python scripts/wino4_loop.py run [--doc F]    # on the GPU: every variant in a child process of its own under `timeout`, stopping at the
                                                  # first one that fails; then the tables go into F between its table markers
                                                  # (default: docs/experiments/wino4_tail.md; wino4_loop.md keeps the tables of its change)
    python scripts/wino4_loop.py one LIB OUT.json # what a child does: time LIB in the three forms under the two loops (and read its stamps)

The variants never go into libpesr_hip.so, and all but `base` and `no_fences` compute wrong results: they are for timing only."""
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
EXP = os.path.join(R, "exp")
VARIANTS = [("base", []), ("stamps", ["-DW4_STAMPS"]), ("no_xform", ["-DW4_NO_XFORM"]), ("no_stload", ["-DW4_NO_STLOAD"]),
            ("no_stage", ["-DW4_NO_XFORM", "-DW4_NO_STLOAD"]), ("no_barrier", ["-DW4_NO_BARRIER"]), ("no_aread", ["-DW4_NO_AREAD"]),
            ("no_wload", ["-DW4_NO_WLOAD"]), ("no_exchange", ["-DW4_NO_EXCHANGE"]), ("mfma_only", ["-DW4_MFMA_ONLY"]),
            ("mfma_only_no_exchange", ["-DW4_MFMA_ONLY", "-DW4_NO_EXCHANGE"]), ("no_fences", ["-DW4_NO_FENCES"])]
WHAT = {"base": "the product", "stamps": "the product with stamps", "no_xform": "no staging transform + LDS stores", "no_stload": "no staging loads",
        "no_stage": "neither of the two", "no_barrier": "no barrier per chunk", "no_aread": "no A-fragment reads", "no_wload": "no weight loads",
        "no_exchange": "no epilogue exchange", "mfma_only": "nothing but the MFMAs in the loop", "mfma_only_no_exchange": "the same, and no exchange",
        "no_fences": "no sched_barrier pairs (right results)"}
FORMS = ("bias + ReLU", "skip", "mask")
LOOPS = ("new", "tail")
LOOP_ENV = {"new": {"PESR_WINO4_TAIL": "0"}, "tail": {}}
LOOP_NAME = {"new": "loop without the TAIL form (`PESR_WINO4_TAIL=0`)", "tail": "loop with the TAIL form"}
N, H, W, C = 16, 48, 48, 256
CHUNKS = C // 16
BEGIN, END = "<!-- wino4_loop.py: tables -->", "<!-- wino4_loop.py: end of tables -->"


def lib_path(name):
    return os.path.join(EXP, f"libw4_{name}.so")


def build(only=()):
    from pesr_amd import build as B
    B.build(verbose=False)                                   # the regular objects, pesr_amd/build/*.o
    os.makedirs(EXP, exist_ok=True)
    hipcc = "hipcc"
    src = os.path.join(B.CSRC, "conv3x3_wino4.hip")
    others = [os.path.join(B.HERE, "build", os.path.basename(s) + ".o") for s in B._sources() if s != src]
    procs = []
    for name, flags in VARIANTS:
        if only and name not in only:
            continue
        obj = os.path.join(EXP, f"w4_{name}.o")
        procs.append((name, obj, subprocess.Popen([hipcc] + B.HIPCC_FLAGS + flags + ["-c", src, "-o", obj])))
    for name, obj, p in procs:
        if p.wait() != 0:
            raise SystemExit(f"hipcc failed on variant {name}")
        subprocess.check_call([hipcc, "-shared", f"--offload-arch={B.ARCH}", "-fPIC", "-o", lib_path(name), obj] + others)
        print(lib_path(name), flush=True)


def one(path, out):
    import numpy as np
    import torch
    from pesr_amd import _lib
    l = ctypes.CDLL(path)
    for name, (res, a) in _lib.SIGNATURES.items():
        if hasattr(l, name):
            f = getattr(l, name); f.restype = res; f.argtypes = a
    dev = "cuda"
    x = torch.rand(N, H, W, C, device=dev) - 0.5
    w = (torch.rand(C, C, 3, 3, device=dev) - 0.5) * 0.1
    b = torch.rand(C, device=dev) - 0.5
    sk = torch.rand(N, H, W, C, device=dev) - 0.5
    mk = torch.rand(N, H, W, C, device=dev) - 0.5
    y = torch.empty(N, H, W, C, device=dev)
    wp = torch.empty(18 * C * C, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    assert l.pesr_pack_conv3x3_wino4(w.data_ptr(), wp.data_ptr(), C, C, 0, 0, s) == 0

    def launch(form):
        skip = sk.data_ptr() if form == "skip" else None
        mask = mk.data_ptr() if form == "mask" else None
        act, alpha = (1, 1.0) if form == "bias + ReLU" else (0, 0.1 if form == "skip" else 1.0)
        rc = l.pesr_conv3x3_wino4(x.data_ptr(), wp.data_ptr(), b.data_ptr(), skip, mask, y.data_ptr(), N, H, W, C, C, alpha, act, 0.0, 0, 0, None, 0, s)
        assert rc == 0, rc

    def timed(form, reps=5, n=100):
        for _ in range(20):
            launch(form)
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                launch(form)
            e1.record(); e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / n)
        return statistics.median(us), min(us), max(us)

    res = {"lib": os.path.basename(path), "us": {}, "stamps": {}}
    for loop in ("tail", "new"):
        os.environ.pop("PESR_WINO4_TAIL", None)
        os.environ.update(LOOP_ENV[loop])
        for form in FORMS:
            res["us"][f"{loop}/{form}"] = timed(form)
            if hasattr(l, "pesr_debug_w4_stamps"):
                torch.cuda.synchronize()
                wgs = 256
                buf = (ctypes.c_ulonglong * (wgs * 8 * 48))()
                l.pesr_debug_w4_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
                assert l.pesr_debug_w4_stamps(buf, wgs) == 0
                t = np.frombuffer(buf, dtype=np.uint64).reshape(wgs * 8, 48).astype(np.int64)
                # s_memtime counts shader clocks from a base of the wave's XCD: differences inside a wave only.  The clock comes from the
                # two s_memrealtime stamps (100 MHz) around the same interval.
                ghz = float(np.median((t[:, 37] - t[:, 0]) / np.maximum(t[:, 39] - t[:, 38], 1) * 0.1))
                us = (t - t[:, :1]) / (ghz * 1000.0)
                rel = [3 + 2 * c for c in range(CHUNKS)]; arr = [2 + 2 * c for c in range(CHUNKS)]
                last = rel[-1]
                ph = {"prologue (entry -> first barrier released)": us[:, 1] - us[:, 0],
                      "loop (-> last chunk barrier released)": us[:, last] - us[:, 1],
                      "  of it: waiting at the 16 chunk barriers": (us[:, rel] - us[:, arr]).sum(1),
                      "  of it: the first chunk": us[:, rel[0]] - us[:, 1],
                      "  of it: the last chunk": us[:, last] - us[:, rel[-2]],
                      "  of it: a middle chunk (mean of chunks 2..15)": (us[:, rel[-2]] - us[:, rel[0]]) / (CHUNKS - 2),
                      "output transform + exchange stores (-> exchange barrier)": us[:, 34] - us[:, last],
                      "waiting at the exchange barrier": us[:, 35] - us[:, 34],
                      "exchange reads, skip / mask loads, epilogue, stores issued": us[:, 36] - us[:, 35],
                      "stores acknowledged": us[:, 37] - us[:, 36],
                      "whole wave (entry -> stores acknowledged)": us[:, 37] - us[:, 0],
                      "shader clock over the wave's life (GHz)": (t[:, 37] - t[:, 0]) / np.maximum(t[:, 39] - t[:, 38], 1) * 0.1}
                if loop == "tail":                       # slots 40 / 42 / 44: a group's exchange barrier released, 41 / 43 / 45: its last store issued
                    ph.update({"TAIL: last chunk's start -> group 0's exchange barrier released": us[:, 40] - us[:, rel[-2]],
                               "TAIL: -> group 1's exchange barrier released": us[:, 42] - us[:, 40],
                               "TAIL: -> group 2's exchange barrier released": us[:, 44] - us[:, 42],
                               "TAIL: group 0's last store issued, behind its barrier": us[:, 41] - us[:, 40],
                               "TAIL: group 1's last store issued, behind its barrier": us[:, 43] - us[:, 42],
                               "TAIL: group 2's last store issued, behind its barrier": us[:, 45] - us[:, 44]})
                res["stamps"][f"{loop}/{form}"] = {k: (float(np.median(v)), float(v.min()), float(v.max())) for k, v in ph.items()}
    with open(out, "w") as fh:
        json.dump(res, fh)


def tables(results):
    base = results["base"]["us"]
    lines = ["### Phases", "",
             "In-kernel stamps (`-DW4_STAMPS`: `s_memtime` shader clocks, turned into us with the median clock that the two `s_memrealtime` stamps",
             "of a wave give), over the 2048 waves of one launch: median (min .. max) in us."]
    st = results.get("stamps", {}).get("stamps", {})
    for loop in LOOPS:
        keys = [f"{loop}/{f}" for f in FORMS if f"{loop}/{f}" in st]
        if not keys:
            continue
        lines += ["", f"The {LOOP_NAME[loop]}:", "", "| phase | " + " | ".join(FORMS) + " |", "|---|" + "---|" * len(FORMS)]
        for ph in st[keys[0]]:
            lines.append(f"| {ph.strip() if not ph.startswith('  ') else '- ' + ph.strip()} | " + " | ".join("%.2f (%.2f .. %.2f)" % tuple(st[k][ph]) for k in keys) + " |")
    lines += ["", "### Ablations", "",
              "HIP-event time per launch, 100 launches back to back, median of five (us); in brackets the difference to the product under the same loop."]
    for loop in LOOPS:
        lines += ["", f"The {LOOP_NAME[loop]}:", "", "| build | " + " | ".join(FORMS) + " |", "|---|" + "---|" * len(FORMS)]
        for name, _ in VARIANTS:
            if name not in results:
                continue
            u = results[name]["us"]
            lines.append(f"| `{name}`: {WHAT[name]} | " + " | ".join("%.1f (%+.1f)" % (u[f"{loop}/{f}"][0], u[f"{loop}/{f}"][0] - base[f"{loop}/{f}"][0]) for f in FORMS) + " |")
    lines += ["", "### The two loops, same library, same process", "",
              "| form | without TAIL | with TAIL | TAIL - without | spread of the five (without / TAIL) |", "|---|---|---|---|---|"]
    for f in FORMS:
        n, t = base[f"new/{f}"], base[f"tail/{f}"]
        lines.append(f"| {f} | {n[0]:.2f} | {t[0]:.2f} | {t[0] - n[0]:+.2f} | {n[2] - n[1]:.2f} / {t[2] - t[1]:.2f} |")
    return "\n".join(lines) + "\n"


def run(doc, only=()):
    global VARIANTS
    if only:
        VARIANTS = [v for v in VARIANTS if v[0] in only]
    out_dir = os.path.join(EXP, "wino4_loop")                 # the children's results, one JSON file per variant
    os.makedirs(out_dir, exist_ok=True)
    results = {}
    for name, _ in VARIANTS:
        if not os.path.exists(lib_path(name)):
            raise SystemExit(f"{lib_path(name)} is missing: python scripts/wino4_loop.py build")
        js = os.path.join(out_dir, name + ".json")
        # one GPU step per variant, each under its own time limit; nothing more is started after one that fails
        rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "one", lib_path(name), js]).returncode
        if rc != 0:
            raise SystemExit(f"variant {name} ended with status {rc}: stopping")
        results[name] = json.load(open(js))
        print(name, {k: round(v[0], 2) for k, v in results[name]["us"].items()}, flush=True)
    text = tables(results)
    print(text)
    body = open(doc).read() if os.path.exists(doc) else f"{BEGIN}\n{END}\n"
    assert BEGIN in body and END in body, f"{doc} has no table markers"
    body = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda m: BEGIN + "\n" + text + END, body, flags=re.S)
    with open(doc, "w") as fh:
        fh.write(body)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "build":
        build(sys.argv[2:])
    elif cmd == "one":
        one(sys.argv[2], sys.argv[3])
    elif cmd == "run":
        run(sys.argv[sys.argv.index("--doc") + 1] if "--doc" in sys.argv else os.path.join(R, "docs", "experiments", "wino4_tail.md"),
            sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else ())
    else:
        raise SystemExit(__doc__)
