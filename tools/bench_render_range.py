"""A batch of different small meshes through the renderer: ONE range-mode call (rasterize(..., ranges=batch.ranges()) -> interpolate ->
antialias, forward and backward) against the loop of B instanced calls that the same batch needs without range mode. The shape is that
of tools/bench_batched.py: B noisy icospheres of frequency 40 (16 002 vertices, 32 000 faces each), one look-at view per mesh, 256 x 256,
for B = 64 and B = 16. Two loops are timed:
    loop_slices   the B calls of the slice law: pos[None] of the union mesh and tri[start_b : start_b + count_b], B different face tensors
                  (more than the 8 the per-tensor caches of the adjacency hold, as with any 64 different meshes: every pass rebuilds them);
    loop_meshes   the B meshes on their own (V_b, 4) positions, all with ONE shared local face tensor (these meshes have one topology): every
                  cache hits, what is left is the launch chain of B small calls.
Each figure is the median over `repeats` rounds of the time between two events around one pass (device time as the stream sees it, idle
gaps of a launch-bound loop included), after warm-up; a round times the three variants one after the other, so they alternate in one
process. Writes one JSON document.
    python tools/bench_render_range.py [out.json] [repeats]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
import largesteps.render as dr
from largesteps import synthetic
from largesteps.batched import MeshBatch
from largesteps.normals import compute_face_normals, compute_vertex_normals

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "render_range_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device("cuda:0")
RES, FREQ = 256, 40


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = x, y, z
    M[:3, 3] = -M[:3, :3] @ eye
    return M


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def case(B):
    v0, f0 = synthetic.icosphere(FREQ)
    vs = [torch.from_numpy(synthetic.perturb(v0, radial=0.03, seed=i)).to(dev) for i in range(B)]
    fs = [torch.from_numpy(f0).to(dev) for _ in range(B)]
    batch = MeshBatch(vs, fs)
    P = dr.persp_proj(45.0, 1.0, 0.1, 100.0).double().numpy()
    mvps = [torch.from_numpy(P @ look_at((3 * np.cos(2 * np.pi * k / B), 0.8 * np.sin(3.0 * k), 3 * np.sin(2 * np.pi * k / B)))).float().to(dev)
            for k in range(B)]
    pos = torch.cat([torch.matmul(torch.nn.functional.pad(v, (0, 1), 'constant', 1.0), m.t()) for v, m in zip(batch.split(batch.verts), mvps)])
    pos = pos.contiguous()
    faces, ranges = batch.faces, batch.ranges()
    attr = (0.5 * compute_vertex_normals(batch.verts, faces, compute_face_normals(batch.verts, faces)) + 0.5).contiguous()
    local = fs[0].long().contiguous()
    slice_faces = [faces[s:s + c].contiguous() for s, c in ranges.tolist()]
    vp = batch.vertex_ptr

    def chain(p, a, tri, **kw):
        rast = dr.rasterize(None, p, tri, (RES, RES), **kw)[0]
        col = dr.interpolate(a, rast, tri)[0]
        return dr.antialias(col, rast, p, tri)

    def leaves():
        return pos.clone().requires_grad_(True), attr.clone().requires_grad_(True)

    def range_call(grad):
        p, a = leaves() if grad else (pos, attr)
        out = chain(p, a, faces, ranges=ranges)
        if grad:
            out.sum().backward()

    def loop_slices(grad):
        p, a = leaves() if grad else (pos, attr)
        for tri in slice_faces:
            out = chain(p[None], a, tri)
            if grad:
                out.sum().backward()

    def loop_meshes(grad):
        p, a = leaves() if grad else (pos, attr)
        for b in range(B):
            out = chain(p[vp[b]:vp[b + 1]][None], a[vp[b]:vp[b + 1]], local)
            if grad:
                out.sum().backward()

    variants = {"range": range_call, "loop_slices": loop_slices, "loop_meshes": loop_meshes}
    res = {"B": B, "V_per_mesh": int(v0.shape[0]), "F_per_mesh": int(f0.shape[0]), "items": int(faces.shape[0])}
    for grad, tag in ((False, "fwd"), (True, "fwd_bwd")):
        ctx = torch.enable_grad() if grad else torch.no_grad()
        with ctx:
            for fn in variants.values():
                for _ in range(2):
                    fn(grad)
            ts = {k: [] for k in variants}
            for _ in range(repeats):
                for k, fn in variants.items():
                    ts[k].append(event_ms(lambda: fn(grad)))
        for k in variants:
            res[f"{k}_{tag}_ms"] = float(np.median(ts[k]))
            res[f"{k}_{tag}_min_max_ms"] = [float(min(ts[k])), float(max(ts[k]))]
        for k in ("loop_slices", "loop_meshes"):
            res[f"{k}_over_range_{tag}"] = res[f"{k}_{tag}_ms"] / res[f"range_{tag}_ms"]
    return res


doc = {"device": torch.cuda.get_device_name(0), "resolution": RES, "icosphere_frequency": FREQ, "repeats": repeats,
       "unit": "ms (median time between events around one pass over all B meshes: rasterize + interpolate + antialias)",
       "loop_slices": "B instanced calls on pos[None] and the B slices of tri (B face tensors: the 8-entry adjacency cache misses)",
       "loop_meshes": "B instanced calls on per-mesh positions with one shared face tensor (every cache hits)", "cases": []}
for B in (64, 16):
    doc["cases"].append(case(B))
    print(json.dumps(doc["cases"][-1]), flush=True)
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(doc, fh, indent=1)
print("wrote", out_path)
