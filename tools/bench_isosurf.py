"""Device time of largesteps.levelset.isosurface (csrc/isosurf.hip) on a 256^3 grid, for two fields: the signed distance of a sphere, and
0.5 - the winding number of the 70k synthetic sphere (what remesh_level_set extracts). Timed: the forward alone, and the forward plus
the backward of the loss sum(V * W) for fixed seeded weights W.

The baseline is what users write today: marching tetrahedra in plain torch on the same device (`torch_marching_tets` below) -- sliced
gathers of the corner signs, a case table, torch.unique over the keys 8 node + slot of the crossed edges, positions by indexing S, the
backward by autograd. The tool checks that both give the same number of vertices and faces and the same vertex set (the sorted edge
keys), and records the largest difference of the positions.

Measurement: `warmup` untimed rounds, then `repeats` rounds in which the two versions alternate in one process, each call between
device events with a device synchronise before and after; median / min / max. Algorithmic bytes are computed from shapes -- the
forward reads S once per pass (count, fill) and writes V, E, F once; the backward reads S and gV once and writes gS once -- and are
reported over the median time. No assertion on speed and no threshold. Writes one JSON document.
    python tools/bench_isosurf.py [out.json] [repeats] [grid side]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch

SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
LONE = {0: (1, 2, 3), 1: (0, 3, 2), 2: (0, 1, 3), 3: (0, 2, 1)}
PAIR = {(0, 1): (2, 3), (0, 2): (3, 1), (0, 3): (1, 2), (1, 2): (0, 3), (1, 3): (2, 0), (2, 3): (0, 1)}


def _case_table():
    """(16, 2, 3) tet edges of the triangles of a positive tet, and (16,) their number: the rule of csrc/isosurf.hip"""
    tris, ntri = np.zeros((16, 2, 3), np.int64), np.zeros(16, np.int64)
    e = lambda x, y: EDGES.index((min(x, y), max(x, y)))
    for case in range(1, 15):
        low = [i for i in range(4) if case >> i & 1]
        high = [i for i in range(4) if not case >> i & 1]
        if len(low) != 2:
            i = low[0] if len(low) == 1 else high[0]
            o = LONE[i] if len(low) == 1 else (LONE[i][0], LONE[i][2], LONE[i][1])
            ntri[case], tris[case, 0] = 1, [e(i, o[0]), e(i, o[1]), e(i, o[2])]
        else:
            (a, b), (c, d) = low, PAIR[tuple(low)]
            ntri[case], tris[case, 0], tris[case, 1] = 2, [e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]
    return tris, ntri


def torch_marching_tets(S, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """(V (n, 3), F (m, 3), keys (n,)) of a finite field S (nx, ny, nz) in plain torch; V is differentiable in S through autograd.
    Vertices come out in the order of the device's (sorted keys); faces are grouped by tet, then cube."""
    dev = S.device
    nx, ny, nz = S.shape
    tris, ntri = (torch.from_numpy(x).to(dev) for x in _case_table())
    low = S.detach() < iso
    ci, cj, ck = torch.meshgrid(torch.arange(nx - 1, device=dev), torch.arange(ny - 1, device=dev), torch.arange(nz - 1, device=dev), indexing="ij")
    base = ((ci * ny + cj) * nz + ck).reshape(-1)
    faces = []
    for t, (a, b, c) in enumerate(PERMS):
        v = np.zeros((4, 3), np.int64)
        v[1, a] = 1
        v[2, a] = v[2, b] = 1
        v[3] = 1
        case = torch.zeros((nx - 1, ny - 1, nz - 1), dtype=torch.int64, device=dev)
        for i in range(4):
            case |= low[v[i, 0]:v[i, 0] + nx - 1, v[i, 1]:v[i, 1] + ny - 1, v[i, 2]:v[i, 2] + nz - 1].to(torch.int64) << i
        case = case.reshape(-1)
        active = torch.nonzero((case != 0) & (case != 15)).reshape(-1)
        case, node0 = case[active], base[active]
        # the key 8 node + slot of every tet edge, for the active tets
        key = torch.stack([8 * (node0 + (v[x, 0] * ny + v[x, 1]) * nz + v[x, 2]) + SLOTS.index(tuple(v[y] - v[x])) for x, y in EDGES], 1)
        odd = (a, b, c) in ((0, 2, 1), (1, 0, 2), (2, 1, 0))
        for j in range(2):
            sel = ntri[case] > j
            tri = tris[case[sel], j]
            if odd:
                tri = tri[:, [0, 2, 1]]
            faces.append(torch.gather(key[sel], 1, tri))
    fkeys = torch.cat(faces)
    keys, inverse = torch.unique(fkeys.reshape(-1), return_inverse=True)
    F = inverse.reshape(-1, 3)
    node, slot = keys // 8, keys % 8
    d = torch.tensor(SLOTS, device=dev)[slot]
    ijk = torch.stack([node // (ny * nz), node // nz % ny, node % nz], 1)
    other = node + (d[:, 0] * ny + d[:, 1]) * nz + d[:, 2]
    Sf = S.reshape(-1)
    t = ((iso - Sf[node]) / (Sf[other] - Sf[node])).clamp(0.0, 1.0)
    o, sp = (torch.tensor(x, dtype=torch.float32, device=dev) for x in (origin, spacing))
    V = o + sp * (ijk.to(torch.float32) + t[:, None] * d.to(torch.float32))
    return V, F, keys


def main():
    from largesteps import synthetic
    from largesteps.distance import MeshDistance
    from largesteps.levelset import isosurface

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "isosurf_bench.json")
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    side = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    warmup = 2
    dev = torch.device("cuda:0")
    shape = (side, side, side)
    N = side ** 3

    def grid(lo, hi):
        axes = [torch.linspace(float(a), float(b), side, dtype=torch.float64, device=dev) for a, b in zip(lo, hi)]
        return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).to(torch.float32)

    def fields():
        lo, hi = np.full(3, -1.0), np.full(3, 1.0)
        P = grid(lo, hi)
        yield "sphere_sdf", ((P - torch.tensor([0.03, -0.02, 0.01], device=dev)).norm(dim=1) - 0.8).reshape(shape), lo, (hi - lo) / (side - 1)
        v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
        v = v.astype(np.float32)
        ext = v.max(0) - v.min(0)
        lo, hi = v.min(0) - 0.05 * ext, v.max(0) + 0.05 * ext
        with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(f, dtype=np.int64)).to(dev)) as mesh:
            S = (0.5 - mesh.winding_number(grid(lo, hi))).to(torch.float32).reshape(shape)
        yield "winding_of_sphere70k", S, lo, (hi - lo) / (side - 1)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ms, nbytes):
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        return {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "algorithmic_bytes": nbytes, "algorithmic_gb_per_s": nbytes / med / 1e6}

    doc = {"device": torch.cuda.get_device_name(0), "grid": list(shape), "repeats": repeats, "warmup": warmup, "cases": []}
    for name, S, lo, sp in fields():
        origin, spacing = tuple(float(x) for x in lo), tuple(float(x) for x in sp)
        S = S.contiguous()
        V, F, E = isosurface(S, 0.0, origin, spacing, return_edges=True)
        Vt, Ft, keys = torch_marching_tets(S, 0.0, origin, spacing)
        assert V.shape == Vt.shape and F.shape == Ft.shape, (V.shape, Vt.shape, F.shape, Ft.shape)
        assert torch.equal(E, keys), "the two versions disagree on the set of crossed edges"
        n, m = int(V.shape[0]), int(F.shape[0])
        W = torch.from_numpy(np.random.default_rng(0).standard_normal((n, 3)).astype(np.float32)).to(dev)
        case = {"field": name, "vertices": n, "faces": m, "largest_position_difference": float((V - Vt).abs().max())}
        del V, F, E, Vt, Ft, keys
        Sg = S.clone().requires_grad_()

        def both(fn):
            Sg.grad = None
            (fn(Sg, 0.0, origin, spacing)[0] * W).sum().backward()
        runs = {"native_forward": lambda: isosurface(S, 0.0, origin, spacing), "torch_forward": lambda: torch_marching_tets(S, 0.0, origin, spacing),
                "native_forward_backward": lambda: both(isosurface), "torch_forward_backward": lambda: both(torch_marching_tets)}
        ms = {k: [] for k in runs}
        for r in range(warmup + repeats):
            for k, fn in runs.items():                       # the versions alternate inside every round
                x = event_ms(fn)
                if r >= warmup:
                    ms[k].append(x)
        fwd = 2 * 4 * N + 12 * n + 8 * n + 24 * m           # S once per pass (count, fill); V, E and F written once
        bwd = 4 * N + 12 * n + 4 * N                        # S and gV read once, gS written once
        for k in runs:
            case[k] = stats(ms[k], fwd + (bwd if k.endswith("backward") else 0))
        case["torch_over_native_forward"] = case["torch_forward"]["median_ms"] / case["native_forward"]["median_ms"]
        case["torch_over_native_forward_backward"] = case["torch_forward_backward"]["median_ms"] / case["native_forward_backward"]["median_ms"]
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
