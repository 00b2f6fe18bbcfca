"""The one recipe that compiles a byte-image kernel file of pesr_amd/csrc as plain C++ into a stand-alone host program
(tests/host_shim: the lanes of a workgroup as threads, __syncthreads as a barrier), for the tests/test_*_host_cpu.py modules.
Nothing is loaded into Python; no GPU is involved."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "host_shim")
CSRC = os.path.join(ROOT, "pesr_amd", "csrc")


def build(name, d, flags=()):
    """csrc/NAME.hip + tests/host_shim/NAME_main.cpp -> (program, d), built in the directory d.  The copy of the kernel file lies next
    to no header, so its "common.h" and "launchers.h" are the shim's; csrc follows on the include path for the shared exact_u8.h.
    flags: further compiler flags, such as -fsanitize=address or -fsanitize=thread for a sanitized build of the program."""
    cxx = shutil.which("clang++") or shutil.which("g++")
    assert cxx, "a host C++20 compiler (clang++ or g++) is needed"
    kernels = os.path.join(str(d), name + "_kernels.cpp")
    shutil.copy(os.path.join(CSRC, name + ".hip"), kernels)
    exe = os.path.join(str(d), name + "_host")
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", *flags, "-I", SHIM, "-I", CSRC,
                    os.path.join(SHIM, name + "_main.cpp"), kernels, "-o", exe, "-pthread"], check=True, capture_output=True, text=True,
                   timeout=300)
    return exe, d


def run(program, parts, timeout=120):
    """Write the call (bytes-like pieces, in main.cpp's order) to in.bin, run the program -> (exit status, out.bin as uint8)."""
    import numpy as np
    exe, d = program
    with open(os.path.join(str(d), "in.bin"), "wb") as f:
        for p in parts:
            f.write(p)
    out = os.path.join(str(d), "out.bin")
    r = subprocess.run([exe, os.path.join(str(d), "in.bin"), out], capture_output=True, text=True, timeout=timeout)
    return r.returncode, np.fromfile(out, dtype=np.uint8)
