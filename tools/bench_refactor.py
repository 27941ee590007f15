"""
Same-pattern refactorisation against construction (include/largesteps_hip.h, ls_direct_refactor), one process, one device:

  per config: median of 10 constructions of NestedDissectionSolver (plain and refactorable), median of 10 refactors (A and B in turn),
              the constructor's stage split (analysis / tables / numeric, seconds), the refactorable handle's kept device bytes, and the
              median solve time (k = 3) of the plain and the refactorable handle;
  a loop on cfg3_dragon250k: the cotangent matrix re-linearised on the current vertices every 50 steps (from_differential + backward),
              through parameterize.update_matrix against a new matrix and a new solver: ms per period of 50 steps.

    python tools/bench_refactor.py [--out file.json] [--configs cfg2_bunny70k,...] [--periods 6]
Prints one JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _matrices(name, dev):
    from largesteps import synthetic
    from largesteps.geometry import compute_matrix
    v, f, c = synthetic.config_mesh(name)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    kw = dict(lambda_=c["lambda_"] if c["lambda_"] is not None else 0.0, alpha=c["alpha"], cotan=c["cotan"])
    A = compute_matrix(tv, tf, **kw)
    if c["cotan"]:
        B = compute_matrix(torch.from_numpy(synthetic.perturb(v, radial=0.01, seed=7).astype(np.float32)).to(dev), tf, **kw)
    else:
        kw["lambda_"] = 1.9 * kw["lambda_"] + 1.0
        B = compute_matrix(tv, tf, **kw)
    return tv, A, B


def _solve_ms(s, b, n=100):
    dev = b.device
    for _ in range(5):
        s.solve(b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(5):
        e0.record()
        for _ in range(n // 5):
            s.solve(b)
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / (n // 5))
    return statistics.median(out)


def bench_config(name, dev, reps=10):
    from largesteps.solvers import NestedDissectionSolver
    tv, A, B = _matrices(name, dev)
    NestedDissectionSolver(A, ordering="longest-axis").close()                   # warm-up: kernels loaded, pool filled
    res = dict(config=name, V=int(A.shape[0]), nnz=int(A._nnz()))
    for label, refac in (("plain", False), ("refactorable", True)):
        ts, stages = [], []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            s = NestedDissectionSolver(A, ordering="longest-axis", refactorable=refac)
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
            stages.append([s.timings["plan_seconds"], s.timings["table_seconds"], s.timings["factor_seconds"]])
            if refac:
                res["retained_device_bytes"] = s.retained_bytes
            s.close()
        res[f"constructor_{label}_median_ms"] = 1e3 * statistics.median(ts)
        res[f"constructor_{label}_stages_median_ms"] = [1e3 * statistics.median(x) for x in zip(*stages)]
    s = NestedDissectionSolver(A, ordering="longest-axis", refactorable=True)
    p = NestedDissectionSolver(A, ordering="longest-axis")
    b = torch.randn((A.shape[0], 3), device=dev)
    res["solve_plain_median_ms"] = _solve_ms(p, b)
    res["solve_refactorable_median_ms"] = _solve_ms(s, b)
    s.refactor(B)
    ts = []
    for i in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s.refactor(A if i % 2 == 0 else B)
        ts.append(time.perf_counter() - t0)
    res["refactor_median_ms"] = 1e3 * statistics.median(ts)
    res["refactor_over_constructor"] = res["refactor_median_ms"] / res["constructor_plain_median_ms"]
    res["solve_after_refactor_median_ms"] = _solve_ms(s, b)
    s.close()
    p.close()
    return res


def bench_relinearise(dev, periods=6, steps=50):
    """cfg3_dragon250k, cotangent matrix on the current vertices every `steps` steps: update_matrix vs a new matrix + a new solver."""
    from largesteps import synthetic
    from largesteps.geometry import compute_matrix
    from largesteps.parameterize import from_differential, to_differential, update_matrix
    v, f, c = synthetic.config_mesh("cfg3_dragon250k")
    tf = torch.from_numpy(f).to(dev)
    kw = dict(lambda_=0.0, alpha=c["alpha"], cotan=True)
    out = {}
    for mode in ("update_matrix", "rebuild"):
        tv = torch.from_numpy(v).to(dev)
        M = compute_matrix(tv, tf, **kw)
        if mode == "update_matrix":
            update_matrix(M, M)
        u = to_differential(M, tv).detach().clone().requires_grad_(True)
        w = torch.randn_like(tv)
        per = []
        for k in range(periods + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            vk = tv + 1e-3 * k * w                                   # "the current vertices"
            M_new = compute_matrix(vk, tf, **kw)
            if mode == "update_matrix":
                M = update_matrix(M, M_new)
            else:
                M = M_new                                             # the old matrix dies, and its solver with it
            for _ in range(steps):
                x = from_differential(M, u)
                (x * w).sum().backward()
                u.grad = None
            torch.cuda.synchronize(dev)
            if k:                                                     # period 0: warm-up
                per.append(1e3 * (time.perf_counter() - t0))
        out[f"{mode}_ms_per_period"] = statistics.median(per)
        del M
    out["steps_per_period"] = steps
    out["speedup"] = out["rebuild_ms_per_period"] / out["update_matrix_ms_per_period"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2_bunny70k,cfg3_dragon250k,cfg4_plane1m,cfg4b_sphere1m")
    ap.add_argument("--periods", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), configs=[bench_config(n, dev) for n in a.configs.split(",") if n],
               relinearise_cfg3_dragon250k=bench_relinearise(dev, a.periods))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
