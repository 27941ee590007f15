"""Device time of largesteps.render (csrc/raster.hip) on the 70k and 1M noisy spheres (cfg2_bunny70k, cfg4b_sphere1m) at 512 x 512,
B = 1 and B = 8 look-at views: forward and backward of rasterize, interpolate and antialias, NVDRenderer.render forward + backward,
and the reference's whole loop body (from_differential -> normals -> render -> L1 -> backward -> AdamUniform) replayed as a captured
graph. Each figure is the median of `repeats` timed runs (CUDA events around `inner` calls, after warm-up). No nvdiffrast figure
exists on this hardware to compare with. Writes one JSON document.
    python tools/bench_render.py [out.json] [repeats]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
import largesteps.render as dr
from largesteps import synthetic
from largesteps.capture import CapturedStep
from largesteps.geometry import compute_matrix
from largesteps.normals import compute_face_normals, compute_vertex_normals
from largesteps.optimize import AdamUniform
from largesteps.parameterize import to_differential, from_differential

out = sys.argv[1] if len(sys.argv) > 1 else "render_bench.json"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
RES = 512


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = x, y, z
    M[:3, 3] = -M[:3, :3] @ eye
    return torch.from_numpy(M).float().to(dev)


def views(B):
    return [look_at((3 * np.cos(2 * np.pi * k / B), 0.8 * np.sin(3.0 * k), 3 * np.sin(2 * np.pi * k / B))) for k in range(B)]


def envmap():
    th = np.linspace(0, np.pi, 32)[:, None]
    ph = np.linspace(0, 2 * np.pi, 64)[None, :]
    e = np.stack([0.6 + 0.4 * np.cos(th) + 0 * ph, 0.5 + 0.3 * np.sin(th) * np.cos(ph), 0.4 + 0.3 * np.cos(2 * th) + 0 * ph,
                  np.ones((32, 64))], -1)
    return torch.from_numpy(e.astype(np.float32)).to(dev)


def timed(fn, inner=5):
    for _ in range(2):
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


doc = {"device": torch.cuda.get_device_name(0), "resolution": RES, "repeats": repeats, "unit": "ms (median device time per call)",
       "comparison": "none: nvdiffrast does not run on ROCm, and no earlier renderer figure exists in this repository", "cases": []}
for name in ("cfg2_bunny70k", "cfg4b_sphere1m"):
    v, f, _ = synthetic.config_mesh(name)
    tv, tf = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
    n = compute_vertex_normals(tv, tf, compute_face_normals(tv, tf))
    for B in (1, 8):
        params = {"res_x": RES, "res_y": RES, "fov": 45.0, "near_clip": 0.1, "far_clip": 100.0, "view_mats": views(B), "envmap": envmap(),
                  "envmap_scale": 1.0}
        R = dr.NVDRenderer(params)
        pos = torch.matmul(torch.nn.functional.pad(tv, (0, 1), 'constant', 1.0), R.mvps.transpose(1, 2)).contiguous()
        light = R.sh.eval(n).contiguous()[None]
        case = {"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "B": B}
        case["rasterize_fwd"] = timed(lambda: dr.rasterize(None, pos, tf, (RES, RES)))
        rast = dr.rasterize(None, pos, tf, (RES, RES))[0]
        case["pixel_order"] = timed(lambda: dr._InstancedFrame(tf.shape[0]).pixel_order(rast, 0))
        p = pos.clone().requires_grad_(True)
        case["rasterize_fwd_bwd"] = timed(lambda: dr.rasterize(None, p, tf, (RES, RES))[0][..., :2].sum().backward())
        case["interpolate_fwd"] = timed(lambda: dr.interpolate(light, rast, tf))
        a = light.clone().requires_grad_(True)
        case["interpolate_fwd_bwd"] = timed(lambda: dr.interpolate(a, rast, tf)[0].sum().backward())
        col = torch.cat((dr.interpolate(light, rast, tf)[0], torch.ones((B, RES, RES, 1), device=dev)), -1)
        case["antialias_fwd"] = timed(lambda: dr.antialias(col, rast, pos, tf))
        c = col.clone().requires_grad_(True)
        case["antialias_fwd_bwd"] = timed(lambda: dr.antialias(c, rast, p, tf).sum().backward())
        vv = tv.clone().requires_grad_(True)
        ref = R.render(tv, n, tf).detach()
        case["render_fwd_bwd"] = timed(lambda: (R.render(vv, n, tf) - ref).abs().mean().backward())
        M = compute_matrix(tv, tf, lambda_=10.0)
        u = to_differential(M, tv).clone().requires_grad_(True)
        opt = AdamUniform([u], 1e-3, capturable=True)

        def body():
            x = from_differential(M, u, 'Cholesky')
            nn = compute_vertex_normals(x, tf, compute_face_normals(x, tf))
            loss = (R.render(x, nn, tf) - ref).abs().mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss
        step = CapturedStep(body, warmup=2)
        case["captured_step"] = timed(step)
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
        del R, step, opt, M
        torch.cuda.empty_cache()
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
print("wrote", out)
