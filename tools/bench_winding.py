"""Device time and accuracy of the winding number and the signed distance of largesteps.distance (csrc/winding.hip) on the 70k and 1M
synthetic spheres, for n = 2^18 query points: area-weighted surface samples moved 1/4, 1 and 4 mean edges along the face normal to
both sides (six equal shares) and a seventh share uniform in the mesh's box grown by half. Timed: `prepare` (the node moments),
`winding_number` at beta = 2, 3 and 4, the exact kernel (all n on the 70k mesh, the first 2^12 on the 1M mesh), `signed_distance` next to
`squared_distance` of the same points. Recorded without any assertion: max and mean |w_beta - w_exact| against the device's own exact
kernel (all n on the 70k mesh, the first 2^14 on the 1M mesh), and how many signs differ from the exact classification. Device events
around each call after `warmup` calls, median / min / max of `repeats`. Writes one JSON document.
    python tools/bench_winding.py [out.json] [repeats] [workload ...]"""
import json
import math
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import _native, synthetic
from largesteps.distance import MeshDistance
from largesteps.sampling import sample_surface

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "winding_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg4b_sphere1m"]
warmup = 3
N = 1 << 18
dev = torch.device("cuda:0")


def timed(fn, n=None):
    """(median, min, max) ms of fn() between device events, after the warm-up calls; Mpoints/s of the median for n points"""
    ms = []
    for k in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    ms.sort()
    res = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
    if n is not None:
        res["mpoints_per_s"] = n / res["median_ms"] / 1e3
    return res


def points(V, F, n):
    """n fp32 query points, shuffled so that every prefix has all seven shares"""
    P, I, _ = sample_surface(V, F, n, seed=1)
    a, b, c = (V[F[I, k]] for k in range(3))
    nrm = torch.nn.functional.normalize(torch.linalg.cross(b - a, c - a), dim=1)
    h = float(((a - b).norm(dim=1) + (b - c).norm(dim=1) + (c - a).norm(dim=1)).mean()) / 3.0
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    share = torch.randint(0, 7, (n,), generator=gen, device=dev)
    off = torch.tensor([0.25, -0.25, 1.0, -1.0, 4.0, -4.0, 0.0], device=dev)[share] * h
    lo, hi = V.min(0).values, V.max(0).values
    box = (lo + hi) / 2 + (torch.rand((n, 3), generator=gen, device=dev) * 1.5 - 0.75) * (hi - lo)
    return torch.where((share == 6)[:, None], box, P + off[:, None] * nrm).contiguous(), h


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "points": N, "cases": []}
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    V = torch.from_numpy(v.astype(np.float32)).to(dev)
    F = torch.from_numpy(f).to(dev)
    big = F.shape[0] > 500000
    with MeshDistance(V, F) as m:
        P, h = points(V, F, N)
        case = {"workload": w, "V": int(V.shape[0]), "F": int(F.shape[0]), "mean_edge": h}
        buf = m._moments()
        lib, st = _native.lib(), _native.stream_of(dev)
        case["prepare"] = timed(lambda: _native.check(lib.ls_mesh_winding_prepare(m._h, _native.ptr(buf), st)))
        n_exact_timed, n_exact_err = (1 << 12, 1 << 14) if big else (N, N)
        case["exact"] = dict(timed(lambda: m.winding_number(P[:n_exact_timed], beta=math.inf), n_exact_timed), points=n_exact_timed)
        we = m.winding_number(P[:n_exact_err], beta=math.inf)
        case["accuracy_points"] = n_exact_err
        for beta in (2.0, 3.0, 4.0):
            row = timed(lambda: m.winding_number(P, beta=beta), N)
            e = (m.winding_number(P[:n_exact_err], beta=beta) - we).abs()
            row.update(max_error=float(e.max()), mean_error=float(e.mean()),
                       signs_that_differ=int(((m.winding_number(P[:n_exact_err], beta=beta) >= 0.5) != (we >= 0.5)).sum()))
            case[f"winding_number_beta_{beta:g}"] = row
        case["exact_range"] = [float(we.min()), float(we.max())]
        case["signed_distance"] = timed(lambda: m.signed_distance(P), N)
        case["squared_distance"] = timed(lambda: m.squared_distance(P), N)
    doc["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
