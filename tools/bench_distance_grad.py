"""Device time of the gradient of largesteps.distance (csrc/distance.hip) on the 70k and 1M synthetic meshes, each queried with the
vertices of a perturbed copy of itself: the forward query; the gradient to P; the gradient to V, in total and split by kernel into the
weights, the group-by (keys, radix sort, segments) and the sums (face rows, vertex gather); `update` against destroy plus create; and a
plain-torch autograd formulation of the same gradient (gather of V[F[I]], weights from the statement's region tests) on the same
inputs in the same process. Device events around each call after `warmup` calls, median / min / max of `repeats`; the per-kernel split
is the kernel durations of torch.profiler summed by name over `repeats` calls. Writes one JSON document.
    python tools/bench_distance_grad.py [out.json] [repeats] [workload ...]"""
import ctypes
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import _native, synthetic
from largesteps.distance import MeshDistance

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "distance_grad_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg4b_sphere1m"]
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


def kernel_split(fn):
    """mean ms per call of the kernels of fn(), by group of kernel names"""
    groups = {"weights": ("k_md_weights",), "group_by": ("k_md_keys", "k_rs_", "k_gb_", "k_scan", "scan"), "sums": ("k_md_face_rows", "k_md_gather_verts")}
    try:
        from torch.profiler import ProfilerActivity, profile
        prof = profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU])
        prof.start()
    except (ImportError, RuntimeError) as exc:            # a machine without a working tracer: the totals above stand alone
        return {"unavailable": repr(exc)}
    try:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
    finally:
        prof.stop()
    res = {g: 0.0 for g in groups}
    res["other"], names = 0.0, {}
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            dur = float(getattr(e, "device_time", getattr(e, "cuda_time", 0.0))) / 1e3 / repeats
            g = next((g for g, keys in groups.items() if any(k in e.name for k in keys)), "other")
            res[g] += dur
            names[e.name[:60]] = names.get(e.name[:60], 0.0) + dur
    res["kernels_ms"] = names
    return res


# ---- the same gradient in plain torch: the region tests of the statement, autograd through the weighted sum ----------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def torch_weights(p, a, b, c):
    """barycentric weights of the closest point (non-degenerate faces), detached: the envelope formulation"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    v_ab, w_ac, w_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = 1.0 / ((va + vb) + vc)
    v, w = vb * den, vc * den
    zero, one = torch.zeros_like(v), torch.ones_like(v)
    out = torch.stack([(1.0 - v) - w, v, w], -1)
    for cond, val in ((((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)), (zero, 1.0 - w_bc, w_bc)),
                      (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), (1.0 - w_ac, zero, w_ac)),
                      (((d6 >= 0) & (d5 <= d6)), (zero, zero, one)),
                      (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), (1.0 - v_ab, v_ab, zero)),
                      (((d3 >= 0) & (d4 <= d3)), (zero, one, zero)),
                      (((d1 <= 0) & (d2 <= 0)), (one, zero, zero))):
        out = torch.where(cond[:, None], torch.stack(val, -1), out)
    return out


def torch_gradients(P, V, F, I, g):
    P, V = P.detach().requires_grad_(), V.detach().requires_grad_()
    corners = V[F[I]].double()                                   # (n, 3, 3)
    p = P.double()
    with torch.no_grad():
        w = torch_weights(p, corners[:, 0], corners[:, 1], corners[:, 2])
    d = p - (w[:, :, None] * corners).sum(1)
    return torch.autograd.grad((g * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])).sum(), (P, V))


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "cases": []}
lib = _native.lib()
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    V = torch.from_numpy(v.astype(np.float32)).to(dev)
    F = torch.from_numpy(f).to(dev)
    P = torch.from_numpy(synthetic.perturb(v, radial=0.01, seed=1).astype(np.float32)).to(dev)
    n = P.shape[0]
    g = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
    with MeshDistance(V, F) as m:
        sqrD, I, C = m.squared_distance(P)
        vptr, order = m._corner_ranks()
        ws = _native.workspace("ls_mesh_distance_backward_workspace_bytes", (n, F.shape[0]), dev)
        gP, gV = torch.empty_like(P), torch.empty_like(V)

        def backward(gp, gv):
            _native.check(lib.ls_mesh_distance_backward(m._h, _native.ptr(P), n, _native.ptr(I), _native.ptr(C), _native.ptr(g), _native.ptr(vptr),
                                                        _native.ptr(order), _native.ptr(gp), _native.ptr(gv), _native.ptr(ws), ws.numel(),
                                                        _native.stream_of(dev)))

        Pg, Vg = P.clone().requires_grad_(), V.clone().requires_grad_()
        m.update(Vg)

        def autograd_step():
            torch.autograd.grad((m.squared_distance(Pg)[0] * g).sum(), (Pg, Vg))

        tP, tV = torch_gradients(P, V, F, I, g)
        backward(gP, gV)
        torch.cuda.synchronize()
        case = {"workload": w, "V": int(V.shape[0]), "F": int(F.shape[0]), "n": int(n), "workspace_bytes": int(ws.numel()),
                "query": timed(lambda: m.squared_distance(P)),
                "grad_P": timed(lambda: backward(gP, None)),
                "grad_V": timed(lambda: backward(None, gV)),
                "grad_V_by_kernel": kernel_split(lambda: backward(None, gV)),
                "forward_backward_autograd": timed(autograd_step),
                "update": timed(lambda: m.update(V)),
                "destroy_create": timed(lambda: MeshDistance(V, F).close()),
                "torch_autograd_gradients": timed(lambda: torch_gradients(P, V, F, I, g)),
                "max_abs_difference_to_torch": {"gP": float((gP - tP).abs().max()), "gV": float((gV - tV).abs().max())}}
    doc["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
