"""Device time of the mipmapped largesteps.render.texture (csrc/mip.hip) at B = 8, 1024 x 1024 pixels, a 2048 x 2048 x 3 texture,
filter_mode='linear-mipmap-linear': forward and backward (gradients to tex, uv, uv_da), against (a) the existing filter_mode='linear'
lookup on the same inputs and (b) a plain-torch trilinear lookup over a torch.nn.functional.avg_pool2d pyramid, written here. uv is a
smooth random warp of the unit square and uv_da a footprint of 0.5 to 16 texels, so every level down to 128 x 128 is read. Each figure is
the median of `repeats` timed runs (device events around `inner` calls, after warm-up; the variants alternate). Writes one JSON document.
    python tools/bench_mip.py [out.json] [repeats]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import torch
import torch.nn.functional as F
import largesteps.render as dr

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "mip_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
RES, B, TS, C = 1024, 8, 2048, 3


def timed(fn, inner=3):
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


def bilinear(t, uv):
    """the 'linear' + 'wrap' lookup in plain torch, differentiable in t and uv; t (1, H, W, C)"""
    Ht, Wt = t.shape[1], t.shape[2]
    x, y = uv[..., 0] * Wt - 0.5, uv[..., 1] * Ht - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0, j0 = torch.remainder(x0.long(), Wt), torch.remainder(y0.long(), Ht)
    i1, j1 = torch.remainder(i0 + 1, Wt), torch.remainder(j0 + 1, Ht)
    t00, t10, t01, t11 = t[0, j0, i0], t[0, j0, i1], t[0, j1, i0], t[0, j1, i1]
    top = t00 + (t10 - t00) * fx
    bot = t01 + (t11 - t01) * fx
    return top + (bot - top) * fy


def torch_trilinear(tex, uv, uv_da):
    """baseline (b): an avg_pool2d pyramid and two masked bilinear lookups per level pair"""
    levels = [tex]
    while levels[-1].shape[1] > 1:
        levels.append(F.avg_pool2d(levels[-1].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    Lmax = len(levels) - 1
    sx, sy, tx, ty = uv_da[..., 0] * TS, uv_da[..., 1] * TS, uv_da[..., 2] * TS, uv_da[..., 3] * TS
    A, Bq, Cc = sx * sx + tx * tx, sy * sy + ty * ty, sx * sy + tx * ty
    m = 0.5 * (A + Bq) + torch.sqrt(0.25 * (A - Bq) ** 2 + Cc * Cc)
    lod = (0.5 * torch.log2(m)).clamp(0, Lmax)
    l0 = torch.floor(lod).clamp(max=Lmax - 1)
    f = (lod - l0)[..., None]
    res = torch.zeros(uv.shape[:3] + (tex.shape[3],), device=uv.device)
    for l in range(int(l0.min()), int(l0.max()) + 1):
        sel = (l0 == l)[..., None]
        c0, c1 = bilinear(levels[l], uv), bilinear(levels[l + 1], uv)
        res = torch.where(sel, c0 + (c1 - c0) * f, res)
    return res


def main():
    g = torch.Generator(device="cpu").manual_seed(0)
    tex = torch.rand((1, TS, TS, C), generator=g).to(dev).requires_grad_(True)
    jj, ii = torch.meshgrid(torch.arange(RES), torch.arange(RES), indexing="ij")
    base = torch.stack([(ii + 0.5) / RES, (jj + 0.5) / RES], -1)
    scale = torch.exp2(torch.linspace(-1.0, 4.0, B))                      # footprint in texels per pixel, per image
    uv = torch.stack([(base - 0.5) * (s * RES / TS) + 0.5 + 0.01 * torch.sin(6.28 * base.flip(-1) * (k + 1)) for k, s in enumerate(scale)]).to(dev)
    uv_da = torch.zeros((B, RES, RES, 4))
    uv_da[..., 0] = uv_da[..., 3] = (scale / TS)[:, None, None]
    uv_da[..., 1] = uv_da[..., 2] = 0.2 * uv_da[..., 0]
    uv_da = uv_da.to(dev)
    uv.requires_grad_(True)
    uv_da.requires_grad_(True)
    gout = torch.rand((B, RES, RES, C), generator=g).to(dev)

    def fwd_mip():
        return dr.texture(tex, uv, uv_da, filter_mode='linear-mipmap-linear')

    def fwd_linear():
        return dr.texture(tex, uv, filter_mode='linear')

    def fwd_torch():
        return torch_trilinear(tex, uv, uv_da)

    def bwd(fn):
        def run():
            tex.grad = uv.grad = uv_da.grad = None
            (fn() * gout).sum().backward()
        return run

    err = float((fwd_mip().detach() - fwd_torch().detach()).abs().max())
    assert err < 1e-4, f"native and plain-torch trilinear lookups differ by {err}"
    doc = {"device": torch.cuda.get_device_name(0), "B": B, "resolution": RES, "tex": [1, TS, TS, C], "repeats": repeats,
           "max_abs_difference_to_plain_torch": err}
    with torch.no_grad():
        mip = dr.texture_construct_mip(tex)
        f = {"mip": [], "mip_prebuilt": [], "linear": [], "torch": []}
        for _ in range(3):
            f["mip"].append(timed(fwd_mip))
            f["mip_prebuilt"].append(timed(lambda: dr.texture(tex, uv, uv_da, mip=mip, filter_mode='linear-mipmap-linear')))
            f["linear"].append(timed(fwd_linear))
            f["torch"].append(timed(fwd_torch, inner=1))
        doc["pyramid_build_ms"] = timed(lambda: dr.texture_construct_mip(tex))
    doc["forward_ms"] = {k: float(np.median(v)) for k, v in f.items()}
    b = {"mip": [], "linear": [], "torch": []}
    for _ in range(2):
        b["mip"].append(timed(bwd(fwd_mip), inner=1))
        b["linear"].append(timed(bwd(fwd_linear), inner=1))
        b["torch"].append(timed(bwd(fwd_torch), inner=1))
    doc["forward_backward_ms"] = {k: float(np.median(v)) for k, v in b.items()}
    doc["ratios"] = {"forward_mip_over_linear": doc["forward_ms"]["mip"] / doc["forward_ms"]["linear"],
                     "forward_mip_prebuilt_over_linear": doc["forward_ms"]["mip_prebuilt"] / doc["forward_ms"]["linear"],
                     "forward_torch_over_mip": doc["forward_ms"]["torch"] / doc["forward_ms"]["mip"],
                     "forward_backward_mip_over_linear": doc["forward_backward_ms"]["mip"] / doc["forward_backward_ms"]["linear"],
                     "forward_backward_torch_over_mip": doc["forward_backward_ms"]["torch"] / doc["forward_backward_ms"]["mip"]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
