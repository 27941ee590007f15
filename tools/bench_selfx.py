"""Device time of the self-intersection queries of largesteps.distance (csrc/selfx.hip) on the 70k and 1M synthetic spheres, each as it is
(clean) and with a tangential jitter of one mean edge (synthetic.perturb(tangential=1.0, seed=5): a mesh that cuts through itself all
over). Timed on one handle per mesh: `count_self_intersections` (one walk per face, no synchronisation), `self_intersections` (count,
one host read of k, the scan, the second walk, the two-word sort) and, for comparison, `squared_distance` of the F face centroids: the
existing walk of the same tree with as many threads. Recorded next to them: the number of pairs and of faces in some pair. No
assertion and no threshold. Device events around each call after `warmup` calls, median / min / max of `repeats`; `self_intersections`
ends in its own synchronise, so its events bracket the whole call. Writes one JSON document.
    python tools/bench_selfx.py [out.json] [repeats] [workload ...]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import synthetic
from largesteps.distance import MeshDistance

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "selfx_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg4b_sphere1m"]
warmup = 3
dev = torch.device("cuda:0")


def timed(fn, n):
    """(median, min, max) ms of fn() between device events, after the warm-up calls; Mfaces/s of the median for n faces"""
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
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "mfaces_per_s": n / ms[len(ms) // 2] / 1e3}


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "cases": []}
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    v = v.astype(np.float32)
    edge = float(np.linalg.norm(v[f[:, 0]].astype(np.float64) - v[f[:, 1]].astype(np.float64), axis=1).mean())
    F = torch.from_numpy(f).to(dev)
    for label, verts in (("clean", v), ("jitter_1.0", synthetic.perturb(v, tangential=1.0, edge=edge, seed=5).astype(np.float32))):
        V = torch.from_numpy(verts).to(dev)
        with MeshDistance(V, F) as m:
            n = int(F.shape[0])
            C = V[F].mean(1).contiguous()
            case = {"workload": w, "mesh": label, "V": int(V.shape[0]), "F": n, "mean_edge": edge,
                    "pairs": int(m.count_self_intersections()), "faces_in_a_pair": int(m.self_intersecting_faces().sum())}
            case["count_self_intersections"] = timed(m.count_self_intersections, n)
            case["self_intersections"] = timed(m.self_intersections, n)
            case["squared_distance_of_centroids"] = timed(lambda: m.squared_distance(C), n)
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
