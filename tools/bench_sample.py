"""Device time of largesteps.sampling (csrc/sample.hip) on the 70k sphere with n = 2^16 and the 1M noisy sphere with n = 2^20: the
forward (ls_sample_surface), the forward plus the gradient to V (ls_sample_surface_backward), the public sample_surface with autograd,
and a plain-torch formulation on the same device in the same process -- fp64 areas, cumsum, torch.rand and searchsorted, gathers, and an
index_add_ backward -- which is the yardstick, never the code under test. Each figure is the time per call of `inner` calls between two
device events, after `warmup` such batches: median / min / max of `repeats`. The per-kernel split is the kernel durations of
torch.profiler summed by name. Writes one JSON document.
    python tools/bench_sample.py [out.json] [repeats] [workload:n ...]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
from largesteps import _native, synthetic
from largesteps.normals import _plan
from largesteps.sampling import sample_surface

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "sample_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k:65536", "cfg4b_sphere1m:1048576"]
warmup, inner = 3, 20
if not torch.cuda.is_available():
    raise SystemExit("bench_sample: no HIP device; nothing is measured without one")
dev = torch.device("cuda:0")


def timed(fn):
    """(median, min, max) ms per call of fn(), `inner` calls between device events, after the warm-up batches"""
    ms = []
    for k in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b) / inner)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def kernel_split(fn):
    """mean ms per call of the kernels of fn(), by name"""
    try:
        from torch.profiler import ProfilerActivity, profile
        prof = profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU])
        prof.start()
    except (ImportError, RuntimeError) as exc:            # a machine without a working tracer: the totals stand alone
        return {"unavailable": repr(exc)}
    try:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
    finally:
        prof.stop()
    names = {}
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            dur = float(getattr(e, "device_time", getattr(e, "cuda_time", 0.0))) / 1e3 / repeats
            names[e.name[:48]] = names.get(e.name[:48], 0.0) + dur
    return names


# ---- the same work in plain torch ------------------------------------------------------------------------------------------------
def torch_forward(V, F, n):
    corners = V[F].double()                                        # (F, 3, 3)
    area = 0.5 * torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).norm(dim=1)
    cum = torch.cumsum(area, 0)
    r = torch.rand((n, 3), dtype=torch.float64, device=V.device)
    I = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp_(max=F.shape[0] - 1)
    s = r[:, 1].sqrt()
    W = torch.stack([1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]], 1).float()
    P = (W[:, :, None] * V[F[I]]).sum(1)
    return P, I, W


def torch_backward(V, F, I, W, gP):
    gV = torch.zeros_like(V)
    gV.index_add_(0, F[I].reshape(-1), (W[:, :, None] * gP[:, None, :]).reshape(-1, 3))
    return gV


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "calls_per_timing": inner, "cases": []}
lib = _native.lib()
for spec in workloads:
    w, n = spec.split(":")
    n = int(n)
    v, f, _ = synthetic.config_mesh(w)
    V = torch.from_numpy(v.astype(np.float32)).to(dev)
    F = torch.from_numpy(f).to(dev)
    nF, nV = F.shape[0], V.shape[0]
    P = torch.empty((n, 3), dtype=torch.float32, device=dev)
    I = torch.empty(n, dtype=torch.int64, device=dev)
    W = torch.empty((n, 3), dtype=torch.float32, device=dev)
    gP = torch.randn((n, 3), dtype=torch.float32, device=dev)
    gV = torch.empty_like(V)
    ws = _native.workspace("ls_sample_workspace_bytes", (nF, n), dev)
    vptr, _, _, order = _plan(F, nV)

    def forward():
        _native.check(lib.ls_sample_surface(_native.ptr(V), _native.ptr(F), F.element_size(), nF, nV, n, 0, 0, 0, _native.ptr(P), _native.ptr(I),
                                            _native.ptr(W), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def backward():
        _native.check(lib.ls_sample_surface_backward(_native.ptr(F), F.element_size(), nF, nV, n, _native.ptr(I), _native.ptr(W), _native.ptr(gP),
                                                     _native.ptr(vptr), _native.ptr(order), _native.ptr(gV), _native.ptr(ws), ws.numel(), dev.index,
                                                     _native.stream_of(dev)))

    def both():
        forward()
        backward()

    Vg = V.clone().requires_grad_()

    def autograd_step():
        torch.autograd.grad((sample_surface(Vg, F, n)[0] * gP).sum(), Vg)

    def torch_both():
        _, tI, tW = torch_forward(V, F, n)
        torch_backward(V, F, tI, tW, gP)

    both()
    ref = torch_backward(V, F, I, W, gP)
    torch.cuda.synchronize()
    case = {"workload": w, "V": int(nV), "F": int(nF), "n": n, "workspace_bytes": int(ws.numel()),
            "forward": timed(forward), "forward_backward": timed(both), "forward_backward_autograd": timed(autograd_step),
            "torch_forward": timed(lambda: torch_forward(V, F, n)), "torch_forward_backward": timed(torch_both),
            "kernels_ms": kernel_split(both),
            "max_abs_difference_of_gV_to_index_add": float((gV - ref).abs().max())}
    case["ratio_torch_over_native"] = {"forward": case["torch_forward"]["median_ms"] / case["forward"]["median_ms"],
                                       "forward_backward": case["torch_forward_backward"]["median_ms"] / case["forward_backward"]["median_ms"]}
    doc["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
