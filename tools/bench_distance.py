"""Device time of largesteps.distance (csrc/distance.hip): MeshDistance construction (LBVH build), the point query (sqrD, I, C of every
vertex of the other mesh), the directed maximum, and the two-sided hausdorff of figures/comparison/generate_data.py, on the 70k, 250k
and 1M-sphere configs, each against a perturbed copy of itself and against a remeshed copy (remesh_botsch, 2 iterations at
h = average edge length). Device events around each call after `warmup` calls; median, min and max of `repeats`. Writes one JSON
document.
    python tools/bench_distance.py [out.json] [repeats] [workload ...]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import synthetic
from largesteps.distance import MeshDistance, hausdorff
from largesteps.meshops import average_edge_length
from largesteps.remesh import remesh_botsch

out = sys.argv[1] if len(sys.argv) > 1 else "distance_bench.json"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg3_dragon250k", "cfg4b_sphere1m"]
warmup = 3
dev = torch.device("cuda:0")


def timed(fn):
    """(median, min, max) ms of fn() between device events, after the warm-up calls"""
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
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "cases": []}
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    tb, tfb = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
    avg = float(average_edge_length(tb, tfb))
    others = {"perturbed": (torch.from_numpy(synthetic.perturb(v, radial=0.01, seed=1).astype(np.float32)).to(dev), tfb),
              "remeshed": remesh_botsch(tb, tfb, 2, avg, True)}
    for kind, (ta, tfa) in others.items():
        with MeshDistance(tb, tfb) as m:
            case = {"workload": w, "against": kind, "V": int(v.shape[0]), "F": int(f.shape[0]), "V_query": int(ta.shape[0]),
                    "F_other": int(tfa.shape[0]),
                    "build": timed(lambda: MeshDistance(tb, tfb).close()),
                    "query": timed(lambda: m.squared_distance(ta)),
                    "max": timed(lambda: m.max_squared_distance(ta)),
                    "kept_hausdorff": timed(lambda: m.hausdorff(ta, tfa)),
                    "hausdorff": timed(lambda: hausdorff(ta, tfa, tb, tfb)),
                    "value": hausdorff(ta, tfa, tb, tfb)}
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
