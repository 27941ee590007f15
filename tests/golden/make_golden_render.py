#!/usr/bin/env python3
"""
Golden fixture for largesteps.render's non-rasterizer parts: EXECUTES the reference's scripts/render.py on the CPU and records what it
computes.
        LARGESTEPS_REFERENCE=<reference checkout> python tests/golden/make_golden_render.py

scripts/render.py imports nvdiffrast (CUDA / OpenGL only) and writes device='cuda' literals. The generator imports it unmodified with
a stub `nvdiffrast.torch` in sys.modules (its `texture` records the coordinates it is handed and returns zeros) and with the device
argument of the torch factory functions it calls redirected from 'cuda' to the CPU; nothing of the file is copied.
Recorded (tests/golden/reference_render.npz, outputs only):
  sh_envmap, sh_M            SphericalHarmonics(envmap).M for a small seeded RGBA environment map
  sh_normals, sh_eval        .eval(n) for seeded unit normals
  proj_args, proj            persp_proj(fov, ar, near, far) for a few argument sets
  bg_view_mats, bg_fov, bg_res, bg_uvs
                             the envmap coordinates NVDRenderer.render_backgrounds hands to texture, for a few views
The archive is written with fixed zip metadata, so the same reference reproduces it byte for byte.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_render.npz")


def _stub_nvdiffrast(record):
    dr = types.ModuleType("nvdiffrast.torch")

    class _Ctx:
        def __init__(self, *a, **k):
            pass

    def texture(tex, uv, *a, **k):
        record.append(uv.detach().clone())
        return torch.zeros((*uv.shape[:-1], tex.shape[-1]), dtype=tex.dtype)

    def _absent(*a, **k):
        raise RuntimeError("not used by the fixture")

    dr.RasterizeGLContext = dr.RasterizeCudaContext = _Ctx
    dr.texture = texture
    dr.rasterize = dr.interpolate = dr.antialias = _absent
    pkg = types.ModuleType("nvdiffrast")
    pkg.torch = dr
    sys.modules["nvdiffrast"] = pkg
    sys.modules["nvdiffrast.torch"] = dr


def _cpu_factories():
    """torch.tensor / linspace / arange / ones / zeros with device='cuda' -> the CPU"""
    for name in ("tensor", "linspace", "arange", "ones", "zeros"):
        fn = getattr(torch, name)

        def wrapped(*a, __fn=fn, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return __fn(*a, **k)
        setattr(torch, name, wrapped)


def _look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = x, y, z
    M[:3, 3] = -M[:3, :3] @ eye
    return M.astype(np.float32)


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = os.environ.get("LARGESTEPS_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        sys.exit("usage: LARGESTEPS_REFERENCE=<reference checkout> python tests/golden/make_golden_render.py")
    record = []
    _stub_nvdiffrast(record)
    _cpu_factories()
    spec = importlib.util.spec_from_file_location("reference_render", os.path.join(ref, "scripts", "render.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    rng = np.random.default_rng(20261016)
    out = {}
    env = rng.uniform(0.0, 2.0, (8, 16, 4)).astype(np.float32)
    sh = R.SphericalHarmonics(torch.from_numpy(env))
    n = rng.standard_normal((32, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    out["sh_envmap"], out["sh_M"] = env, sh.M.numpy()
    out["sh_normals"], out["sh_eval"] = n, sh.eval(torch.from_numpy(n)).numpy()

    args = np.array([[45.0, 1.0, 0.1, 100.0], [30.0, 4.0 / 3.0, 0.5, 20.0], [60.0, 0.75, 0.01, 1000.0]])
    out["proj_args"] = args
    out["proj"] = np.stack([R.persp_proj(*a).numpy() for a in args])

    views = np.stack([_look_at((0.0, 0.0, -3.0)), _look_at((2.0, 1.0, 1.5)), _look_at((-1.0, -2.5, 0.5))])
    res = (10, 14)                               # (H, W)
    params = {"res_x": res[1], "res_y": res[0], "fov": 40.0, "near_clip": 0.1, "far_clip": 100.0,
              "view_mats": [torch.from_numpy(m) for m in views], "envmap": torch.from_numpy(env), "envmap_scale": 1.0}
    R.NVDRenderer(params)
    out["bg_view_mats"], out["bg_fov"], out["bg_res"] = views, np.array(40.0), np.array(res)
    out["bg_uvs"] = record[-1].numpy()
    _save(OUT, out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
