"""Record what the nested-dissection solve computes and launches on the cases of tests/direct_launch_cases.py (needs the GPU):

    LARGESTEPS_HIP_LIB=<library of the commit to record> python tools/record_direct_launch_bits.py [out.npz]

writes tests/golden/direct_launch_bits.npz: per case the sha256 of x for k = 1 .. 4, info()'s (launches, tier levels, tier workgroups,
levels) and the (lo, hi, sweep) rows of launch_profile() after a solve with "profile" = 3; for the sharded cases also the digest of the
summed exchange and each rank's shape, cut level and part-1 rows. tests/test_direct_launches_gpu.py compares every later build against
it. The committed record was taken with the library of the commit BEFORE the solve's launches became one list built at create
(csrc/direct.hip, Launch): that change, and any later one of the same kind, must move neither a bit of x nor a row of the reports.
Record again only when a change is MEANT to change the launches or the arithmetic, and say so in the commit.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import direct_launch_cases as dc                    # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", dc.GOLDEN)
    dev = torch.device("cuda:0")
    rec = {}

    def env(case):
        dc.set_env(case, os.environ.__setitem__, lambda name: os.environ.pop(name, None))

    for case in dc.CASES:
        env(case)
        M, B = dc.system(case, dev)
        r = dc.run_unsharded(case, M, B)
        rec[case + "/shape"] = np.array(dc.shape_of(r["inf"]), dtype=np.int64)
        rec[case + "/profile"] = dc.profile_rows(r["prof"])
        for k in dc.KS:
            assert np.array_equal(r["x"][k].view(np.uint32), r["x_profiled"][k].view(np.uint32)), "the profiled solve differs"
            rec[f"{case}/k{k}"] = dc.digest(r["x"][k])
        print(case, rec[case + "/shape"].tolist(), rec[case + "/profile"].tolist(), rec[case + "/k3"].tobytes().hex()[:16], flush=True)
    for case in dc.SHARDED:
        env(case)
        M, B = dc.system(case, dev)
        for exchange in dc.EXCHANGE:
            r = dc.run_sharded(case, M, B, exchange)
            key = f"{case}/{exchange}"
            rec[key + "/shape"] = np.array(r["shape"], dtype=np.int64)
            rec[key + "/cut"] = np.array(r["cut"], dtype=np.int64)
            for rank, rows in enumerate(r["profile"]):
                rec[f"{key}/profile{rank}"] = rows
            for k in dc.KS:
                assert np.array_equal(r["x"][k].view(np.uint32), r["x_profiled"][k].view(np.uint32)), "the profiled solve differs"
                rec[f"{key}/k{k}"] = dc.digest(r["x"][k])
                rec[f"{key}/exchange{k}"] = dc.digest(r["exch"][k])
            print(key, r["shape"], r["cut"], [p.tolist() for p in r["profile"]], rec[key + "/k3"].tobytes().hex()[:16], flush=True)
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
