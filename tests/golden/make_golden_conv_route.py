"""Writes conv_route_trace.json: the kernel launches of the scenarios of tests/conv_route_scenarios.py - every launch entry point of the
library in order, with its integer / float arguments, null or non-null per pointer and the stream it went to - as issued by the
commit this script is run at.  It was run on an MI355X at the commit BEFORE pesr_amd/functional.py routed the forward, the input
gradient and the weight gradient of its conv nodes through three shared functions, when every autograd Function chose its kernels
itself; tests/test_conv_route_gpu.py holds the routers to that recording.  Needs the GPU.
Run from the repository root: python tests/golden/make_golden_conv_route.py [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import conv_route_scenarios as S  # noqa: E402


def main():
    traces = {}
    for sc in S.scenarios():
        traces[sc[0]], _ = S.run(sc)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_route_trace.json")
    packed = S.pack_traces(traces)
    with open(out, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in traces.items()}, "distinct calls:", len(packed["calls"]))


if __name__ == "__main__":
    main()
