"""Wall time of remesh_botsch (largesteps.remesh, csrc/remesh.hip): a 5-iteration call at h = s * average_edge_length on the 70k,
250k and 1M-sphere configs, s in {0.5, 1.0}. Per case: warm-up calls, then `repeats` timed calls (the call synchronises); the median
wall time with its min / max, the per-phase host wall time and round counts of the median call, and V', F'. Writes one JSON document.
    python tools/bench_remesh_botsch.py [out.json] [repeats] [workload ...]"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import synthetic
from largesteps.meshops import average_edge_length
from largesteps.remesh import RemeshHandle

out = sys.argv[1] if len(sys.argv) > 1 else "remesh_bench.json"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg3_dragon250k", "cfg4b_sphere1m"]
dev = torch.device("cuda:0")
doc = {"device": torch.cuda.get_device_name(0), "iterations": 5, "repeats": repeats, "warmup": 2, "cases": []}
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    tv, tf = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
    avg = float(average_edge_length(tv, tf))
    for s in (0.5, 1.0):
        runs = []
        for k in range(2 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with RemeshHandle(tv, tf, s * avg, True) as r:
                r.run(5)
                V, F = r.result()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                info = r.info()
            if k >= 2:
                runs.append((dt, info))
        runs.sort(key=lambda x: x[0])
        ms = [1e3 * d for d, _ in runs]
        med_t, med = runs[len(runs) // 2]
        case = {"workload": w, "V": int(v.shape[0]), "F": int(f.shape[0]), "h_over_avg": s, "median_ms": 1e3 * med_t, "min_ms": ms[0],
                "max_ms": ms[-1], "all_ms": ms, "phase_ms": {k: 1e3 * x for k, x in med["seconds"].items()}, "rounds": med["rounds"],
                "ops": med["ops"], "V_out": med["V"], "F_out": med["F"]}
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
