"""SHA-256 of every tensor the scenarios of tests/conv_route_scenarios.py compute (outputs, input gradients, parameter gradients,
post-step parameters) -> a JSON file; two trees compute the same bits iff their files are equal.
python scripts/conv_route_dump.py OUT.json [TREE]     TREE: root of the checkout whose pesr_amd is imported (default: this one)"""
import hashlib, json, os, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import conv_route_scenarios as S
res = {}
for sc in S.scenarios():
    _, out = S.run(sc)
    for k, t in out.items():
        t = t.detach().contiguous().cpu()
        res[f"{sc[0]}/{k}"] = [list(t.shape), str(t.dtype), hashlib.sha256(t.numpy().tobytes()).hexdigest()]
json.dump(res, open(sys.argv[1], "w"), indent=0)
import pesr_amd
print(len(res), "tensors from", os.path.dirname(pesr_amd.__file__))
