"""Every entry point that sits on the radix sort (csrc/radix.h), the group-by and the segmented sum (csrc/groupby.h), run on fixed
inputs with the library LARGESTEPS_HIP_LIB points at; each output is written as .npy. Two libraries compute the same thing when the
two directories hold the same bytes:
    LARGESTEPS_HIP_LIB=a.so python tools/dump_sort_users.py dump out_a
    LARGESTEPS_HIP_LIB=b.so python tools/dump_sort_users.py dump out_b        (a fresh process each: the library is loaded once)
    python tools/dump_sort_users.py compare out_a out_b                        (exit status 1 when a file differs or is missing)
Covered: remove_duplicates; the CSR transpose of an unsymmetric matrix (backward of to_differential); corner_ranks through the
normals, forward and backward; rasterize / interpolate / antialias forward and every gradient; texture forward and both gradients in
every filter x boundary mode; hausdorff; one remesh_botsch iteration; the direct solver's first solve on the 70k mesh. The renderer's
shapes hold faces and texels with more than 64 pixels and with fewer (asserted: per face from the rast ids of both images, per texel
from the nearest texel of every pixel), so both arms of the segmented sum are compared."""
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"MISSING  {n}")
            bad += 1
            continue
        x, y = np.load(pa), np.load(pb)
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        print(f"{'equal   ' if same else 'DIFFERS '} {n} {x.dtype} {x.shape}")
        bad += not same
    print(f"{len(names)} files, {bad} differ or are missing")
    return 1 if bad or not names else 0


def dump(out):
    import torch
    import largesteps.render as dr
    from largesteps import synthetic
    from largesteps.distance import hausdorff
    from largesteps.geometry import compute_matrix
    from largesteps.meshops import remove_duplicates
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    from largesteps.parameterize import to_differential, from_differential
    from largesteps.remesh import remesh_botsch

    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)

    def save(name, t):
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        np.save(os.path.join(out, name + ".npy"), np.ascontiguousarray(a))

    def dev_f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    def weights(t):
        return dev_f32(rng.standard_normal(tuple(t.shape)))

    v70, f70, cfg70 = synthetic.config_mesh("cfg2_bunny70k")
    v70 = v70.astype(np.float32)

    # ---- remove_duplicates: the shuffled face soup of the 70k mesh
    soup = v70[f70.reshape(-1)]
    order = rng.permutation(soup.shape[0])
    inv = np.empty_like(order)
    inv[order] = np.arange(order.shape[0])
    vu, fu, dup = remove_duplicates(torch.from_numpy(soup[order]).to(dev), torch.from_numpy(inv.reshape(-1, 3)).to(dev))
    save("dedup_verts", vu), save("dedup_faces", fu), save("dedup_inverse", dup)

    # ---- normals (corner_ranks), forward and backward
    tv, tf = torch.from_numpy(v70).to(dev).requires_grad_(True), torch.from_numpy(f70).to(dev)
    fn = compute_face_normals(tv, tf)
    vn = compute_vertex_normals(tv, tf, fn)
    (vn * weights(vn)).sum().backward()
    save("normals_face", fn), save("normals_vertex", vn), save("normals_grad_verts", tv.grad)

    # ---- the CSR transpose: rows of the system matrix scaled one by one make it unsymmetric
    vs, fs = synthetic.icosphere(24)
    vs = synthetic.perturb(vs, radial=0.05, seed=1).astype(np.float32)
    tvs, tfs = torch.from_numpy(vs).to(dev), torch.from_numpy(fs).to(dev)
    M = compute_matrix(tvs, tfs, lambda_=10.0).coalesce()
    scale = dev_f32(1.0 + rng.random(vs.shape[0]))
    L = torch.sparse_coo_tensor(M.indices(), M.values() * scale[M.indices()[0]], M.shape).coalesce()
    x = tvs.clone().requires_grad_(True)
    u = to_differential(L, x)
    (u * weights(u)).sum().backward()
    save("transpose_u", u), save("transpose_grad_v", x.grad)

    # ---- the direct solver: first solve on the 70k mesh
    tv0 = torch.from_numpy(v70).to(dev)
    M70 = compute_matrix(tv0, tf, cfg70["lambda_"])
    save("direct_first_solve", from_differential(M70, to_differential(M70, tv0), "Cholesky"))

    # ---- hausdorff and one remesh_botsch iteration
    va, fa = synthetic.icosphere(32)
    vb = synthetic.perturb(va, radial=0.05, seed=2).astype(np.float32)
    va = va.astype(np.float32)
    save("hausdorff", np.float64(hausdorff(torch.from_numpy(va).to(dev), torch.from_numpy(fa).to(dev), torch.from_numpy(vb).to(dev),
                                           torch.from_numpy(fa).to(dev))))
    vr, fr = remesh_botsch(torch.from_numpy(vb).to(dev), torch.from_numpy(fa).to(dev).int(), 1, 0.05, True)
    save("remesh_verts", vr), save("remesh_faces", fr)

    # ---- rasterize / interpolate / antialias: a sphere of small faces in front of two large triangles, two views
    vi, fi = synthetic.icosphere(8)
    nv = vi.shape[0]
    quad = np.array([[-0.9, -0.9, 0.5], [0.9, -0.9, 0.5], [0.9, 0.9, 0.5], [-0.9, 0.9, 0.5]])
    P = np.concatenate([0.6 * vi, quad])
    tri = np.concatenate([fi, np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]])]).astype(np.int32)
    pos = []
    for ang in (0.3, 1.1):
        c, s = np.cos(ang), np.sin(ang)
        Q = P.copy()
        Q[:nv] = P[:nv] @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
        pos.append(np.concatenate([Q, 1.0 + 0.2 * Q[:, 2:3]], 1))
    pos = dev_f32(np.stack(pos)).requires_grad_(True)
    ttri = torch.from_numpy(tri).to(dev)
    attr = dev_f32(rng.random((P.shape[0], 3))).requires_grad_(True)
    rast, _ = dr.rasterize(None, pos, ttri, (128, 128))
    color, _ = dr.interpolate(attr, rast, ttri)
    aa = dr.antialias(color, rast, pos, ttri)
    for ids in rast[..., 3].detach().cpu().numpy().astype(np.int64).reshape(2, -1):
        per_face = np.bincount(ids, minlength=tri.shape[0] + 1)[1:]
        assert per_face.max() > 64 and 0 < per_face[per_face > 0].min() < 64, "the scene must hold faces of more and of fewer than 64 pixels"
    ((aa * weights(aa)).sum() + (rast[..., :2] * weights(rast[..., :2])).sum()).backward()
    save("raster_rast", rast), save("raster_color", color), save("raster_aa", aa), save("raster_grad_pos", pos.grad), save("raster_grad_attr", attr.grad)

    # ---- texture: 8 x 8 texels under 2 x 64 x 64 pixels (hundreds of pixels a texel) and 256 x 256 texels (mostly none or one)
    uv_np = rng.random((2, 64, 64, 2)) * 2.0 - 0.5
    for Ht, C in ((8, 3), (256, 6)):
        tex_np = rng.random((1, Ht, Ht, C))
        for filt in ("nearest", "linear"):
            for bnd in ("wrap", "clamp", "zero"):
                tex, uv = dev_f32(tex_np).requires_grad_(True), dev_f32(uv_np).requires_grad_(True)
                o = dr.texture(tex, uv, filter_mode=filt, boundary_mode=bnd)
                if filt == "nearest" and bnd == "wrap":         # pixels per texel: the nearest texel, wrapped
                    ij = np.floor(uv.detach().cpu().numpy().astype(np.float32) * np.float32(Ht)).astype(np.int64) % Ht
                    hits = np.bincount((ij[..., 1] * Ht + ij[..., 0]).ravel(), minlength=Ht * Ht)
                    assert (hits.min() > 64) if Ht == 8 else (0 < hits[hits > 0].max() < 64), f"texels of {Ht} x {Ht}: {hits.min()} .. {hits.max()} pixels"
                (o * weights(o)).sum().backward()
                tag = f"texture_{Ht}_{filt}_{bnd}"
                save(tag + "_out", o), save(tag + "_grad_tex", tex.grad)
                save(tag + "_grad_uv", uv.grad if uv.grad is not None else torch.zeros_like(uv))
    torch.cuda.synchronize()
    print(f"wrote {len(os.listdir(out))} files to {out} with {os.environ.get('LARGESTEPS_HIP_LIB', 'the package library')}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
