"""Device time of largesteps.subdivide (csrc/subdiv.hip): one level of Loop subdivision of the 70k sphere (cfg2_bunny70k) and of the 1M
noisy sphere (cfg4b_sphere1m) of largesteps.synthetic, positions (V, 3): Subdivision.apply, and apply with its backward, against the
same S built once as a torch.sparse_csr_tensor (from the handle's own edges and flags, on the host) and applied with torch.sparse.mm,
its backward autograd's, on the same device, the two alternating in one process. Also the time of the constructor (the topology: two
radix sorts, two scans, one synchronisation). Each figure is the median of `repeats` timed runs (device events around `inner` calls,
after warm-up). Writes one JSON document. No speed threshold belongs to it: the feature is gated by its bitwise tests.
    python tools/bench_subdivide.py [out.json] [repeats]"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import synthetic
from largesteps.subdivide import Subdivision

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "subdivide_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")


def timed(fn, inner=5):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def loop_matrix(sub, V):
    """Loop's S (V + E, V) as CSR on the device, fp32, from the handle's arrays: Warren's weights"""
    tri, he, edges, opp, valence, bflag, bnbr, _, _ = (a.cpu().numpy() for a in sub._levels[0].arrays)
    E = edges.shape[0]
    rows, cols, vals = [], [], []

    def add(r, c, w):
        rows.append(np.asarray(r, dtype=np.int64))
        cols.append(np.asarray(c, dtype=np.int64))
        vals.append(np.broadcast_to(np.float64(w), rows[-1].shape) if np.ndim(w) == 0 else np.asarray(w, dtype=np.float64))
    e = np.arange(E)
    interior = opp[:, 1] >= 0
    for k in (0, 1):
        add(V + e, edges[:, k], np.where(interior, 0.375, 0.5))
        add(V + e[interior], opp[interior, k], 0.125)
    v = np.arange(V)
    bnd = bflag != 0
    n = valence.astype(np.float64)
    beta = np.where(valence == 3, 3.0 / 16.0, 3.0 / (8.0 * np.maximum(n, 1.0)))
    add(v, v, np.where(valence == 0, 1.0, np.where(bnd, 0.75, 1.0 - n * beta)))
    for k in (0, 1):
        add(v[bnd], bnbr[bnd, k], 0.125)
        ok = ~bnd[edges[:, k]]                               # an interior end takes beta of the other end
        add(edges[ok, k], edges[ok, 1 - k], beta[edges[ok, k]])
    S = torch.sparse_coo_tensor(np.stack([np.concatenate(rows), np.concatenate(cols)]), np.concatenate(vals), (V + E, V)).coalesce()
    return S.to(torch.float32).to_sparse_csr().to(dev)


def main():
    doc = {"device": torch.cuda.get_device_name(0), "scheme": "loop", "levels": 1, "channels": 3, "repeats": repeats, "meshes": {}}
    for name in ("cfg2_bunny70k", "cfg4b_sphere1m"):
        v, f, _ = synthetic.config_mesh(name)
        V = v.shape[0]
        tf = torch.from_numpy(f).to(dev)
        X = torch.from_numpy(v).to(dev).requires_grad_()
        sub = Subdivision(tf, V)
        S = loop_matrix(sub, V)
        g = torch.rand((sub.num_vertices, 3), generator=torch.Generator().manual_seed(0)).to(dev)
        y_native, y_sparse = sub.apply(X).detach(), torch.sparse.mm(S, X).detach()
        err = float((y_native - y_sparse).abs().max())
        assert err < 1e-5, f"{name}: native and sparse results differ by {err}"

        def build():
            Subdivision(tf, V)

        def both(fn):
            def run():
                X.grad = None
                (fn() * g).sum().backward()
            return run
        runs = {"native_apply": lambda: sub.apply(X.detach()), "sparse_apply": lambda: torch.sparse.mm(S, X.detach()),
                "native_apply_backward": both(lambda: sub.apply(X)), "sparse_apply_backward": both(lambda: torch.sparse.mm(S, X))}
        ms = {k: [] for k in runs}
        for _ in range(3):                                   # the variants alternate
            for k, fn in runs.items():
                ms[k].append(timed(fn))
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build()
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        m = {k: float(np.median(x)) for k, x in ms.items()}
        doc["meshes"][name] = {"vertices": V, "faces": int(f.shape[0]), "edges": sub.num_vertices - V, "max_abs_difference_to_sparse": err,
                               "ms": m, "constructor_wall_ms": float(np.median(walls)),
                               "sparse_over_native": {"apply": m["sparse_apply"] / m["native_apply"],
                                                      "apply_backward": m["sparse_apply_backward"] / m["native_apply_backward"]}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
