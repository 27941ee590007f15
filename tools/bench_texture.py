"""Device time of largesteps.render.texture (csrc/texture.hip) at B = 8, 1024 x 1024 pixels: (a) a 1024 x 2048 x 4 environment map
looked up at NVDRenderer.background_uvs(), (b) a 1024 x 1024 x 3 texture looked up at the uv that `interpolate` gives for a spherical
uv attribute on cfg2_bunny70k. Per case: forward (and the plain-torch lookup it replaced, on the same inputs in the same process, the
two alternating), the pixel order, backward to uv, backward to tex with a cached and with a fresh order; the bytes of each by the model
of DESIGN.md section 2.7 and the fraction of the 8 TB/s peak they amount to. Each figure is the median of `repeats` timed runs (device
events around `inner` calls, after warm-up). Writes one JSON document.
    python tools/bench_texture.py [out.json] [repeats]"""
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

out = sys.argv[1] if len(sys.argv) > 1 else "texture_bench.json"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
RES, B = 1024, 8
PEAK = 8.0e12


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


def byte_model(N, Bt, Ht, Wt, C):
    """DESIGN.md section 2.7 (linear filtering): bytes each stage asks the memory system for"""
    T, K = Bt * Ht * Wt, Bt * (Ht + 1) * (Wt + 1)
    passes = 1 if K < 256 else 2 if K < 65536 else 3 if K < (1 << 24) else 4
    return {
        "forward": N * (8 + 16 * C + 4 * C),                                        # uv, four taps, one write
        "order": 4 * N * (8 + 5 * passes) + 4 * K * (1 + math.ceil(math.log2(N))),  # keys, radix passes, sorted keys; segment searches
        "backward_uv": N * (8 + 16 * C + 4 * C + 8),                                # uv, four taps, the gradient row, one write
        "backward_tex": 4 * N * (4 + 8 + 4 * C) + T * (32 + 4 * C),                 # per (pixel, tap): id, uv, gradient row; per texel: segments, one write
    }


def measure(name, tex, uv):
    Bt, Ht, Wt, C = tex.shape
    N = uv.shape[0] * uv.shape[1] * uv.shape[2]
    case = {"case": name, "tex": list(tex.shape), "uv": list(uv.shape)}
    # forward: native and the plain-torch lookup alternate, so that drift of the machine hits both
    assert torch.equal(dr.texture(tex, uv), dr._texture_cpu(tex, uv)), "native and plain-torch lookups differ"
    nat, old = [], []
    for _ in range(3):
        nat.append(timed(lambda: dr.texture(tex, uv)))
        old.append(timed(lambda: dr._texture_cpu(tex, uv), inner=2))
    case["forward"], case["forward_plain_torch"] = float(np.median(nat)), float(np.median(old))
    case["forward_speedup"] = case["forward_plain_torch"] / case["forward"]
    filt, bnd = 1, 0
    case["order"] = timed(lambda: dr._TexelOrder(None).get(uv, Bt, Ht, Wt, filt, bnd))
    g = torch.randn(uv.shape[:3] + (C,), device=dev)
    order, seg = dr._TexelOrder(None).get(uv, Bt, Ht, Wt, filt, bnd)
    gt, gu = torch.empty_like(tex), torch.empty_like(uv)
    lib, nv = dr._native.lib(), dr._native

    def backward(want_tex, want_uv, fresh):
        o, s = dr._TexelOrder(None).get(uv, Bt, Ht, Wt, filt, bnd) if fresh else (order, seg)
        nv.check(lib.ls_texture_backward(nv.ptr(tex), Bt, Ht, Wt, C, nv.ptr(uv), uv.shape[0], uv.shape[1], uv.shape[2], filt, bnd, nv.ptr(g),
                                         nv.ptr(o), nv.ptr(s), nv.ptr(gt if want_tex else None), nv.ptr(gu if want_uv else None), 0,
                                         nv.stream_of(dev)))

    case["backward_uv"] = timed(lambda: backward(False, True, False))
    case["backward_tex_cached_order"] = timed(lambda: backward(True, False, False))
    case["backward_tex_fresh_order"] = timed(lambda: backward(True, False, True))
    t = tex.clone().requires_grad_(True)
    c = uv.clone().requires_grad_(True)
    case["autograd_fwd_bwd_both"] = timed(lambda: (dr.texture(t, c) * g).sum().backward())
    model = byte_model(N, Bt, Ht, Wt, C)
    case["bytes"] = model
    case["fraction_of_8TBps"] = {
        "forward": model["forward"] / (case["forward"] * 1e-3) / PEAK,
        "order": model["order"] / (case["order"] * 1e-3) / PEAK,
        "backward_uv": model["backward_uv"] / (case["backward_uv"] * 1e-3) / PEAK,
        "backward_tex_cached_order": model["backward_tex"] / (case["backward_tex_cached_order"] * 1e-3) / PEAK,
        "backward_tex_fresh_order": (model["backward_tex"] + model["order"]) / (case["backward_tex_fresh_order"] * 1e-3) / PEAK,
    }
    print(json.dumps(case), flush=True)
    return case


doc = {"device": torch.cuda.get_device_name(0), "resolution": RES, "B": B, "repeats": repeats, "unit": "ms (median device time per call)",
       "comparison": "forward: the plain-torch lookup this kernel replaced (largesteps.render._texture_cpu on device tensors); "
                     "backward: none exists", "cases": []}
rng = np.random.default_rng(0)
views = [look_at((3 * np.cos(2 * np.pi * k / B), 0.8 * np.sin(3.0 * k), 3 * np.sin(2 * np.pi * k / B))) for k in range(B)]
small = torch.from_numpy(rng.uniform(0, 1, (8, 16, 4)).astype(np.float32)).to(dev)
R = dr.NVDRenderer({"res_x": RES, "res_y": RES, "fov": 45.0, "near_clip": 0.1, "far_clip": 100.0, "view_mats": views, "envmap": small,
                    "envmap_scale": 1.0})
env = torch.from_numpy(rng.uniform(0, 1, (1, 1024, 2048, 4)).astype(np.float32)).to(dev)
doc["cases"].append(measure("envmap 1024 x 2048 x 4 at background_uvs()", env, R.background_uvs().contiguous()))

v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
tv, tf = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev)
d = tv / tv.norm(dim=1, keepdim=True)
attr = torch.stack([0.5 + torch.atan2(d[:, 0], d[:, 2]) / (2 * np.pi), torch.acos(d[:, 1].clamp(-1, 1)) / np.pi], dim=1).contiguous()
pos = torch.matmul(torch.nn.functional.pad(tv, (0, 1), 'constant', 1.0), R.mvps.transpose(1, 2)).contiguous()
rast = dr.rasterize(None, pos, tf, (RES, RES))[0]
uv = dr.interpolate(attr, rast, tf)[0].contiguous()
tex = torch.from_numpy(rng.uniform(0, 1, (1, 1024, 1024, 3)).astype(np.float32)).to(dev)
case = measure("texture 1024 x 1024 x 3 at interpolate(uv attribute) on cfg2_bunny70k", tex, uv)
case["covered_pixels"] = int((rast[..., 3] > 0).sum())
case["rasterize_fwd_same_frame"] = timed(lambda: dr.rasterize(None, pos, tf, (RES, RES)))
doc["cases"].append(case)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
print("wrote", out)
