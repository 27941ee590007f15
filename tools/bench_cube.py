"""Device time of largesteps.render.texture(..., boundary_mode='cube') (csrc/cube.hip) at B = 8, 1024 x 1024 pixels, a 6 x 512 x 512 cube
with C = 3 and C = 4, looked up along the view rays of eight cameras around the origin (every face and every seam is hit). Per case:
forward, the item order, backward to uv, backward to tex with a cached and with a fresh order, and forward + backward through autograd.
Baseline, in the same process and alternating with the cube calls: the 2-D `linear` + `clamp` lookup (csrc/texture.hip) of the same
texels laid out as one 512 x 3072 texture, at the uv that lands every pixel on the texel cell its cube lookup reads -- the same number
of pixels, the same taps but for the seams. Each figure is the median of `repeats` timed runs (device events around `inner` calls, after
warm-up). Writes one JSON document.
    python tools/bench_cube.py [out.json] [repeats]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
import largesteps.render as dr

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "cube_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
RES, B, N_FACE = 1024, 8, 512
lib, nv = dr._native.lib(), dr._native


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


def view_rays():
    """(B, RES, RES, 3): the rays of a 90-degree camera through every pixel centre, the cameras turning around two axes"""
    t = (2.0 * torch.arange(RES, device=dev, dtype=torch.float32) + 1.0) / RES - 1.0
    y, x = torch.meshgrid(t, t, indexing="ij")
    ray = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    rays = []
    for k in range(B):
        a, e = 2 * np.pi * k / B + 0.3, 0.9 * np.sin(3.0 * k)
        Ry = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32, device=dev)
        Rx = torch.tensor([[1, 0, 0], [0, np.cos(e), -np.sin(e)], [0, np.sin(e), np.cos(e)]], dtype=torch.float32, device=dev)
        rays.append(ray @ (Ry @ Rx).T)
    return torch.stack(rays).contiguous()


def flat_uv(d):
    """the uv of the 512 x 3072 strip (faces side by side) that lands a pixel on the cell its cube lookup reads"""
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    isx, isy = (ax >= ay) & (ax >= az), ay >= az
    ma = torch.where(isx, x, torch.where(isy, y, z))
    face = torch.where(isx, 0, torch.where(isy, 2, 4)) + (ma < 0)
    sc = torch.where(isx, torch.where(x < 0, z, -z), torch.where(isy, x, torch.where(z < 0, -x, x)))
    tc = torch.where(isx, -y, torch.where(isy, torch.where(y < 0, -z, z), -y))
    s, t = (sc / ma.abs() + 1.0) * 0.5, (tc / ma.abs() + 1.0) * 0.5
    return torch.stack([(face + s) / 6.0, t], dim=-1).contiguous(), face


def measure(C, dirs, uv2, rng):
    cube = torch.from_numpy(rng.uniform(0, 1, (1, 6, N_FACE, N_FACE, C)).astype(np.float32)).to(dev)
    strip = cube[0].permute(1, 0, 2, 3).reshape(1, N_FACE, 6 * N_FACE, C).contiguous()
    g = torch.randn(dirs.shape[:3] + (C,), device=dev)
    Bn, H, W, _ = dirs.shape
    case = {"C": C, "cube": list(cube.shape), "strip": list(strip.shape), "pixels": [Bn, H, W]}
    filt = 1
    c_order, c_seg = dr._CubeOrder(None).get(dirs, 1, N_FACE, filt)
    t_order, t_seg = dr._TexelOrder(None).get(uv2, 1, N_FACE, 6 * N_FACE, filt, 1)
    gc, gs, gd, gu = torch.empty_like(cube), torch.empty_like(strip), torch.empty_like(dirs), torch.empty_like(uv2)

    def cube_backward(want_tex, want_uv, fresh):
        o, s = dr._CubeOrder(None).get(dirs, 1, N_FACE, filt) if fresh else (c_order, c_seg)
        nv.check(lib.ls_cube_backward(nv.ptr(cube), 1, N_FACE, C, nv.ptr(dirs), Bn, H, W, filt, nv.ptr(g), nv.ptr(o), nv.ptr(s),
                                      nv.ptr(gc if want_tex else None), nv.ptr(gd if want_uv else None), 0, nv.stream_of(dev)))

    def flat_backward(want_tex, want_uv, fresh):
        o, s = dr._TexelOrder(None).get(uv2, 1, N_FACE, 6 * N_FACE, filt, 1) if fresh else (t_order, t_seg)
        nv.check(lib.ls_texture_backward(nv.ptr(strip), 1, N_FACE, 6 * N_FACE, C, nv.ptr(uv2), Bn, H, W, filt, 1, nv.ptr(g), nv.ptr(o),
                                         nv.ptr(s), nv.ptr(gs if want_tex else None), nv.ptr(gu if want_uv else None), 0, nv.stream_of(dev)))

    tc_, t2 = cube.clone().requires_grad_(True), strip.clone().requires_grad_(True)
    stages = {
        "forward": (lambda: dr.texture(cube, dirs, boundary_mode="cube"), lambda: dr.texture(strip, uv2, boundary_mode="clamp")),
        "order": (lambda: dr._CubeOrder(None).get(dirs, 1, N_FACE, filt), lambda: dr._TexelOrder(None).get(uv2, 1, N_FACE, 6 * N_FACE, filt, 1)),
        "backward_uv": (lambda: cube_backward(False, True, False), lambda: flat_backward(False, True, False)),
        "backward_tex_cached_order": (lambda: cube_backward(True, False, False), lambda: flat_backward(True, False, False)),
        "backward_tex_fresh_order": (lambda: cube_backward(True, False, True), lambda: flat_backward(True, False, True)),
        "backward_both_fresh_order": (lambda: cube_backward(True, True, True), lambda: flat_backward(True, True, True)),
        "backward_both_cached_order": (lambda: cube_backward(True, True, False), lambda: flat_backward(True, True, False)),
        "autograd_fwd_bwd_tex": (lambda: (dr.texture(tc_, dirs, boundary_mode="cube") * g).sum().backward(),
                                 lambda: (dr.texture(t2, uv2, boundary_mode="clamp") * g).sum().backward()),
    }
    for name, (cube_fn, flat_fn) in stages.items():
        a, b = [], []
        for _ in range(3):                      # the two alternate, so that drift of the machine hits both
            a.append(timed(cube_fn))
            b.append(timed(flat_fn))
        case[name] = {"cube": float(np.median(a)), "flat_2d": float(np.median(b)), "ratio": float(np.median(a) / np.median(b))}
    print(json.dumps(case), flush=True)
    return case


dirs = view_rays()
uv2, face = flat_uv(dirs)
doc = {"device": torch.cuda.get_device_name(0), "resolution": RES, "B": B, "n": N_FACE, "repeats": repeats,
       "unit": "ms (median device time per call)", "faces_hit": torch.bincount(face.flatten(), minlength=6).tolist(),
       "baseline": "flat_2d: largesteps.render.texture(strip, uv, 'linear', 'clamp') on the same texels as one 512 x 3072 texture, "
                   "uv aimed at the cell the cube lookup reads; items per pixel: cube 4, flat_2d 1",
       "cases": []}
rng = np.random.default_rng(0)
for C in (3, 4):
    doc["cases"].append(measure(C, dirs, uv2, rng))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(doc, fh, indent=1)
print("wrote", out)
