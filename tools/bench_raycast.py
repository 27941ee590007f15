"""Device time of largesteps.raycast (csrc/raycast.hip) on the 70k and 1M synthetic spheres, for two ray sets of 512 x 512 rays each:
camera rays (coherent: a pinhole camera at (0, 0, 3) looking at the mesh, one ray per pixel centre) and cosine-weighted rays from
area-weighted surface samples around the inward normal (incoherent; every ray ends on the mesh). Timed: `intersect`, `occluded`,
forward plus backward (gradients to O, D and V through autograd), next to them the same handle's `squared_distance` on as many points
(the ray origins; the existing walk, the yardstick) and, for the camera rays, `render.rasterize` of the same view at 512 x 512. Recorded
without any assertion: how many camera-ray face ids differ from rasterize's. Device events around each call after `warmup` calls,
median / min / max of `repeats`. Writes one JSON document.
    python tools/bench_raycast.py [out.json] [repeats] [workload ...]"""
import json
import math
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
import largesteps.render as dr
from largesteps import synthetic
from largesteps.raycast import RayMesh
from largesteps.sampling import sample_surface

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "raycast_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
workloads = sys.argv[3:] or ["cfg2_bunny70k", "cfg4b_sphere1m"]
warmup = 3
RES = 512
dev = torch.device("cuda:0")


def timed(fn, n=None):
    """(median, min, max) ms of fn() between device events, after the warm-up calls; Mrays/s of the median for n rays"""
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
        res["mrays_per_s"] = n / res["median_ms"] / 1e3
    return res


def camera(V):
    """(O, D (RES^2, 3), clip-space positions (1, V, 4)) of a pinhole camera at (0, 0, 3) looking down -z: focal length 2.5, pixel (i, j)
    at NDC ((j + 0.5) 2 / RES - 1, (i + 0.5) 2 / RES - 1), as rasterize places its pixel centres"""
    focal, near, far = 2.5, 0.5, 10.0
    eye = torch.tensor([0.0, 0.0, 3.0], device=dev)
    c = ((torch.arange(RES, device=dev, dtype=torch.float32) + 0.5) * (2.0 / RES) - 1.0) / focal
    D = torch.stack([c[None, :].expand(RES, RES), c[:, None].expand(RES, RES), torch.full((RES, RES), -1.0, device=dev)], -1).reshape(-1, 3).contiguous()
    O = eye.expand_as(D).contiguous()
    pv = V - eye
    pos = torch.stack([focal * pv[:, 0], focal * pv[:, 1], (far + near) / (near - far) * pv[:, 2] + 2.0 * far * near / (near - far), -pv[:, 2]], -1)
    return O, D, pos[None].contiguous()


def surface_rays(V, F, n):
    """n cosine-weighted rays from area-weighted samples, around the inward face normal, started 1e-4 diagonals inside"""
    P, I, _ = sample_surface(V, F, n, seed=1)
    a, b, c = (V[F[I, k]] for k in range(3))
    N = torch.nn.functional.normalize(torch.linalg.cross(b - a, c - a), dim=1)
    N = torch.where(((N * P).sum(1) > 0)[:, None], -N, N)              # a sphere around the origin: inward is towards it
    axis = torch.nn.functional.one_hot(N.abs().argmin(1), 3).to(N.dtype)
    t1 = torch.nn.functional.normalize(torch.linalg.cross(N, axis), dim=1)
    t2 = torch.linalg.cross(N, t1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    u = torch.rand((n, 2), generator=gen, device=dev)
    r, phi = u[:, 0].sqrt(), 2.0 * math.pi * u[:, 1]
    D = (r * phi.cos())[:, None] * t1 + (r * phi.sin())[:, None] * t2 + (1.0 - u[:, 0]).sqrt()[:, None] * N
    diag = float((V.max(0).values - V.min(0).values).norm())
    return (P + 1e-4 * diag * N).contiguous(), D.contiguous()


doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "warmup": warmup, "rays": RES * RES, "cases": []}
for w in workloads:
    v, f, _ = synthetic.config_mesh(w)
    V = torch.from_numpy(v.astype(np.float32)).to(dev)
    F = torch.from_numpy(f).to(dev)
    n = RES * RES
    with RayMesh(V, F) as m:
        Oc, Dc, pos = camera(V)
        Os, Ds = surface_rays(V, F, n)
        case = {"workload": w, "V": int(V.shape[0]), "F": int(F.shape[0])}
        for name, O, D in (("camera", Oc, Dc), ("surface", Os, Ds)):
            t, I, _ = m.intersect(O, D)
            Og, Dg, Vg = O.clone().requires_grad_(), D.clone().requires_grad_(), V.clone().requires_grad_()
            m.update(Vg)

            def forward_backward():
                tt, II, _ = m.intersect(Og, Dg)
                torch.autograd.grad(torch.where(II >= 0, tt, torch.zeros_like(tt)).sum(), (Og, Dg, Vg))

            row = {"hit_fraction": float((I >= 0).float().mean()),
                   "intersect": timed(lambda: m.intersect(O, D), n),
                   "occluded": timed(lambda: m.occluded(O, D), n),
                   "forward_backward": timed(forward_backward, n),
                   "squared_distance_of_the_origins": timed(lambda: m.squared_distance(O), n)}
            m.update(V)
            if name == "camera":
                tri = F.to(torch.int32)
                row["rasterize_512"] = timed(lambda: dr.rasterize(None, pos, tri, (RES, RES)), n)
                rast, _ = dr.rasterize(None, pos, tri, (RES, RES))
                ids = rast[0, :, :, 3].reshape(-1).to(torch.int64) - 1
                row["face_ids_that_differ_from_rasterize"] = int((ids != I).sum())
                row["pixels_covered_by_rasterize"] = int((ids >= 0).sum())
            case[name] = row
    doc["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
