"""Golden fixture GV13 for seeded construction, made by IMPORTING THE REFERENCE (make_golden.import_reference).

Run:  python tests/golden/make_golden_seeded.py          (a few seconds)

  GV13  torch.manual_seed(3), then the reference's Generator({'depth': 2, 'num_channels': 16, 'res_scale': 0.1}) and
        Discriminator({'patch_size': 8, 'spectral_norm': False}) (reference model/pesr.py): every state_dict entry of both, in
        the reference's key order (`keys`, `G|<key>` / `D|<key>`), with its dtype, shape and the sha256 of its contiguous bytes
        (`dtypes`, `shapes` padded with -1, `sha256`), and the values themselves (`<entry>`) of entries up to SMALL elements -
        the parameters the reference's own initialisation gives, bit for bit, for tests/test_entrypoints_cpu.py to compare the
        drop-in modules' construction against.
Only data is written (keys and values) - no reference source text.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (torchvision stub + reference import)

SEED = 3
G_OPT = {"depth": 2, "num_channels": 16, "res_scale": 0.1}
D_OPT = {"patch_size": 8, "spectral_norm": False}
SMALL = 16384


def main():
    ref_model, _ = MG.import_reference()
    torch.manual_seed(SEED)
    G, D = ref_model.Generator(G_OPT), ref_model.Discriminator(D_OPT)
    arrs, keys, dtypes, shapes, digests = {}, [], [], [], []
    for tag, m in (("G", G), ("D", D)):
        for k, v in m.state_dict().items():
            a = v.detach().contiguous().numpy()
            keys.append(f"{tag}|{k}")
            dtypes.append(str(a.dtype))
            shapes.append(list(a.shape) + [-1] * (4 - a.ndim))
            digests.append(hashlib.sha256(a.tobytes()).hexdigest())
            if a.size <= SMALL:
                arrs[f"{tag}|{k}"] = a.copy()
    arrs.update(keys=np.array(keys), dtypes=np.array(dtypes), shapes=np.array(shapes, dtype=np.int64), sha256=np.array(digests),
                seed=np.int64(SEED))
    out = os.path.join(HERE, "gv13_seeded_construction.npz")
    np.savez_compressed(out, **arrs)
    print(out, len(keys), "entries", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
