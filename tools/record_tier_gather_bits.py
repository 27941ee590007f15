"""Record what the tier kernels compute, bit for bit, on the cases of tests/tier_gather_cases.py (needs the GPU):

    LARGESTEPS_HIP_LIB=<library of the commit to record> python tools/record_tier_gather_bits.py [out.npz]

writes tests/golden/tier_gather_bits.npz: per case the sha256 of x and the solver's shape (launches, tier levels, tier workgroups).
tests/test_tier_gather_gpu.py compares every later build against it. The committed record was taken with the library of the commit
BEFORE the tier's gathers were rewritten (load all children, sum by select): that rewrite, and any later one of the same kind, must
not change a bit. Record again only when a change is MEANT to change the arithmetic, and say so in the commit.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import tier_gather_cases as tc                      # noqa: E402
from largesteps.geometry import compute_matrix      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", tc.GOLDEN)
    dev = torch.device("cuda:0")
    rec = {}
    systems = {}
    for name, arity, waves in tc.SHAPES:
        if name not in systems:
            v, f = tc.mesh(name)
            tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
            systems[name] = (compute_matrix(tv, tf, tc.LAMBDA), torch.from_numpy(tc.rhs(v.shape[0])).to(dev))
        M, B = systems[name]
        s = tc.solver(M, arity, waves)
        inf = s.info()
        for k in tc.KS:
            x = s.solve(B[:, :k].contiguous())
            again = s.solve(B[:, :k].contiguous())
            assert torch.equal(x, again), "the solve is not reproducible"
            cid = tc.case_id(name, arity, waves, k)
            rec[cid] = tc.digest(x.cpu().numpy())
            rec[cid + "/shape"] = np.array([inf["launches"], inf["tier_levels"], inf["tier_workgroups"], inf["levels"]], dtype=np.int64)
            print(cid, rec[cid].tobytes().hex()[:16], rec[cid + "/shape"].tolist(), flush=True)
        s.close()
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
