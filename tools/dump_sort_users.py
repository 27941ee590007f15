"""Every entry point that sits on the radix sort (csrc/radix.h), the group-by and the segmented sum (csrc/groupby.h), run on fixed
inputs with the library LARGESTEPS_HIP_LIB points at; each output is written as .npy. Two libraries compute the same thing when the
two directories hold the same bytes:
    LARGESTEPS_HIP_LIB=a.so python tools/dump_sort_users.py dump out_a
    LARGESTEPS_HIP_LIB=b.so python tools/dump_sort_users.py dump out_b        (a fresh process each: the library is loaded once)
    python tools/dump_sort_users.py compare out_a out_b                        (exit status 1 when a file differs or is missing)
Covered: remove_duplicates; the CSR transpose of an unsymmetric matrix (backward of to_differential); corner_ranks through the
normals, forward and backward; rasterize / interpolate / antialias forward and every gradient; texture forward and both gradients in
every filter x boundary mode; the mipmapped lookup (both mip modes x the boundary modes x uv_da, bias or both x a pyramid given or
built in the call) and the cube lookup (both filters, directions across seams and at corners), forward and every gradient, each for
1, 4 and 5 channels (one channel group, the float4 rows, two groups); hausdorff; one remesh_botsch iteration; the direct solver's
first solve on the 70k mesh. The renderer's shapes hold faces and texels with more than 64 pixels and with fewer (asserted: per face
from the rast ids of both images, per texel from the nearest texel of every pixel, per pyramid and cube texel from the item order
itself), so both arms of the segmented sum are compared.
The queries over one mesh and its LBVH (csrc/lbvh.h, meshbvh.h) on the 70k mesh: squared_distance with both gradients, the closest
point's weights, max_squared_distance, RayMesh.intersect with its three gradients and occluded, winding_number at beta = 2 and exact,
the hierarchy and the node moments, signed_distance with its gradients, sample_surface with its vertex gradient, chamfer_distance
with both gradients, and the distance again after one update. The query points are 2^16 surface samples pushed along the normal to
both sides with a share uniform in the grown box, and 1024 more around one face's centroid, so that some face owns more than 64 points
and some face between 1 and 64 (asserted): both arms of the segmented sum again.
With the pairs of self_intersections on two icospheres that cross, the isosurface of a noisy ball on a 24^3 grid with its gradient in
the field, and massmatrix_voronoi and average_edge_length with their gradients, every entry point that carves a caller's workspace
(csrc/workspace.h) is in the comparison; the handle's own buffer and the bisection's are under the mesh queries and the direct solve."""
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

    def grad_or_zero(x):
        return x.grad if x.grad is not None else torch.zeros_like(x)

    # ---- mipmapped texture: the same two sizes; uv_da spreads the pixels' footprints over every level, the bias alone does too
    def mip_items_per_texel(seg, Ht, Lmax):
        """wrap mode, one batch entry: texel i of a level gets the items of base positions i and i - 1 (wrapped) along each axis"""
        cnt, k, per = np.diff(seg.cpu().numpy().astype(np.int64)), 0, []
        for l in range(Lmax + 1):
            h = max(Ht >> l, 1)
            c = cnt[k:k + (h + 1) * (h + 1)].reshape(h + 1, h + 1)[1:, 1:]
            k += (h + 1) * (h + 1)
            per.append((c + np.roll(c, 1, 0) + np.roll(c, 1, 1) + np.roll(np.roll(c, 1, 0), 1, 1)).ravel())
        return np.concatenate(per)

    for Ht in (8, 256):
        Lfull = int(np.log2(Ht))
        da_np = rng.standard_normal((2, 64, 64, 4)) * 2.0 ** rng.uniform(-1.0, Lfull + 1.0, (2, 64, 64, 1)) / Ht
        lod_inputs = {"both": (da_np, rng.uniform(-1.0, 1.0, (2, 64, 64))), "da": (da_np, None),
                      "bias": (None, rng.uniform(-1.0, Lfull + 1.0, (2, 64, 64)))}
        for C in (1, 4, 5):
            tex_np = rng.random((1, Ht, Ht, C))
            for mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
                for bnd in ("wrap", "clamp", "zero"):
                    for how, (da_a, bias_a) in lod_inputs.items():
                        for prebuilt in (False, True):
                            tex, uv = dev_f32(tex_np).requires_grad_(True), dev_f32(uv_np).requires_grad_(True)
                            da = None if da_a is None else dev_f32(da_a).requires_grad_(True)
                            bias = None if bias_a is None else dev_f32(bias_a).requires_grad_(True)
                            mip = dr.texture_construct_mip(tex) if prebuilt else None
                            o = dr.texture(tex, uv, uv_da=da, mip_level_bias=bias, mip=mip, filter_mode=mode, boundary_mode=bnd)
                            (o * weights(o)).sum().backward()
                            if bnd == "wrap" and C == 1 and not prebuilt:
                                items = mip_items_per_texel(uv._largesteps_mip_order.seg, Ht, Lfull)
                                assert items.max() > 64 and (Ht == 8 or 0 < items[items > 0].min() <= 64), \
                                    f"texels of the {Ht} x {Ht} pyramid: {items.min()} .. {items.max()} items"
                            tag = f"mip_{Ht}_c{C}_{mode.split('-')[-1]}_{bnd}_{how}_{'given' if prebuilt else 'built'}"
                            save(tag + "_out", o), save(tag + "_grad_tex", tex.grad), save(tag + "_grad_uv", grad_or_zero(uv))
                            if da is not None:
                                save(tag + "_grad_uv_da", grad_or_zero(da))
                            if bias is not None:
                                save(tag + "_grad_bias", grad_or_zero(bias))

    # ---- cube map: 4 x 4 faces under 2 x 64 x 64 directions (hundreds of items a texel) and 64 x 64 faces (mostly none or a few);
    # the last 512 directions of each image hug the 8 corners and the 12 edges, so taps cross seams and one of four is dropped
    dirs_np = rng.standard_normal((2, 64 * 64, 3))
    near = rng.integers(0, 2, (2, 512, 3)) * 2.0 - 1.0
    near[:, 256:, :] *= np.where(rng.integers(0, 3, (2, 256, 1)) == np.arange(3), rng.uniform(-1.0, 1.0, (2, 256, 1)), 1.0)      # edges
    dirs_np[:, -512:] = (near + 0.02 * rng.standard_normal(near.shape)) * rng.uniform(0.5, 2.0, (2, 512, 1))
    dirs_np = dirs_np.reshape(2, 64, 64, 3)
    for n in (4, 64):
        for C in (1, 4, 5):
            tex_np = rng.random((1, 6, n, n, C))
            for filt in ("nearest", "linear"):
                tex, d = dev_f32(tex_np).requires_grad_(True), dev_f32(dirs_np).requires_grad_(True)
                o = dr.texture(tex, d, filter_mode=filt, boundary_mode="cube")
                (o * weights(o)).sum().backward()
                items = np.diff(d._largesteps_cube_order.seg.cpu().numpy().astype(np.int64))      # keyed by destination texel
                assert (items.max() > 64) if n == 4 else (0 < items[items > 0].min() <= 64), f"texels of 6 x {n} x {n}: {items.min()} .. {items.max()} items"
                tag = f"cube_{n}_c{C}_{filt}"
                save(tag + "_out", o), save(tag + "_grad_tex", tex.grad), save(tag + "_grad_uv", grad_or_zero(d))
    # ---- the mesh queries: one handle over the 70k mesh
    import math
    from largesteps import _native
    from largesteps.distance import chamfer_distance
    from largesteps.raycast import RayMesh
    from largesteps.sampling import sample_surface

    V70, n = torch.from_numpy(v70).to(dev), 1 << 16
    S, SI, _ = sample_surface(V70, tf, n, seed=1)
    a, b, c = (V70[tf[SI, k]] for k in range(3))
    nrm = torch.nn.functional.normalize(torch.linalg.cross(b - a, c - a), dim=1)
    h = float(((a - b).norm(dim=1) + (b - c).norm(dim=1) + (c - a).norm(dim=1)).mean()) / 3.0
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    share = torch.randint(0, 7, (n,), generator=gen, device=dev)
    off = torch.tensor([0.25, -0.25, 1.0, -1.0, 4.0, -4.0, 0.0], device=dev)[share] * h
    lo, hi = V70.min(0).values, V70.max(0).values
    box = (lo + hi) / 2 + (torch.rand((n, 3), generator=gen, device=dev) * 1.5 - 0.75) * (hi - lo)
    near = V70[tf[0].long()].mean(0) + dev_f32(rng.standard_normal((1024, 3))) * (0.05 * h)
    P = torch.cat([torch.where((share == 6)[:, None], box, S + off[:, None] * nrm), near]).contiguous()
    save("query_points", P)
    D = ((lo + hi) / 2 - P) + dev_f32(rng.standard_normal(tuple(P.shape))) * (0.1 * float((hi - lo).norm()))

    def grads(loss, *xs):
        return [g if g is not None else torch.zeros_like(x) for g, x in zip(torch.autograd.grad(loss, xs, allow_unused=True), xs)]

    Vg, Pg = V70.clone().requires_grad_(True), P.clone().requires_grad_(True)
    with RayMesh(Vg, tf) as m:
        sqrD, I, C = m.squared_distance(Pg)
        per_face = np.bincount(I.cpu().numpy(), minlength=f70.shape[0])
        assert per_face.max() > 64 and 0 < per_face[per_face > 0].min() <= 64, "the points must give faces of more and of fewer than 64 points"
        gP, gV = grads((sqrD * weights(sqrD).double()).sum(), Pg, Vg)
        save("distance_sqrD", sqrD), save("distance_I", I), save("distance_C", C), save("distance_grad_P", gP), save("distance_grad_V", gV)
        W = torch.empty((P.shape[0], 3), dtype=torch.float64, device=dev)
        m._call("ls_mesh_distance_weights", _native.ptr(P), P.shape[0], _native.ptr(I), _native.ptr(W))
        save("distance_weights", W), save("distance_max", m.max_squared_distance(P))

        Og, Dg = P.clone().requires_grad_(True), D.clone().requires_grad_(True)
        t, RI, RW = m.intersect(Og, Dg)
        hit = RI >= 0
        print(f"rays: {int(hit.sum())} of {hit.shape[0]} hit, at most {int(np.bincount(RI[hit].cpu().numpy()).max())} on one face")
        gO, gD, gV = grads((torch.where(hit, t, torch.zeros_like(t)) * weights(t).double()).sum(), Og, Dg, Vg)
        save("ray_t", t), save("ray_I", RI), save("ray_W", RW), save("ray_grad_O", gO), save("ray_grad_D", gD), save("ray_grad_V", gV)
        save("ray_occluded", m.occluded(P, D))

        save("winding_beta2", m.winding_number(P, 2.0)), save("winding_exact", m.winding_number(P[:1 << 12], math.inf))
        T70 = f70.shape[0]
        i32 = dict(dtype=torch.int32, device=dev)
        arrays = dict(left=torch.zeros(T70 - 1, **i32), right=torch.zeros(T70 - 1, **i32), esc=torch.zeros(2 * T70 - 1, **i32), tri=torch.zeros(T70, **i32),
                      box=torch.zeros((2 * T70 - 1, 6), dtype=torch.float32, device=dev), mom=torch.zeros((2 * T70 - 1, 36), dtype=torch.float64, device=dev))
        m._call("ls_mesh_winding_arrays", _native.ptr(m._moments()), *(_native.ptr(x) for x in arrays.values()))
        for name, x in arrays.items():
            save("lbvh_" + name, x)
        Sd, _, _ = m.signed_distance(Pg)
        gP, gV = grads((Sd * weights(Sd).double()).sum(), Pg, Vg)
        save("signed_distance", Sd), save("signed_distance_grad_P", gP), save("signed_distance_grad_V", gV)

        V2 = dev_f32(synthetic.perturb(v70.astype(np.float64), radial=0.02, seed=3))
        m.update(V2)
        sqrD, I, C = m.squared_distance(P)
        save("updated_sqrD", sqrD), save("updated_I", I), save("updated_C", C)

    SP, SI, SW = sample_surface(Vg, tf, n, seed=5)
    gV, = grads((SP * weights(SP)).sum(), Vg)
    per_face = np.bincount(SI.cpu().numpy(), minlength=f70.shape[0])
    print(f"samples: at most {per_face.max()} on one face")
    save("sample_P", SP), save("sample_I", SI), save("sample_W", SW), save("sample_grad_V", gV)
    # a mesh of few faces: every face draws far more than 64 samples, the wave-strided arm of the fp64 segmented sum
    vq, fq = synthetic.icosphere(2)
    Vq, Fq = dev_f32(vq).requires_grad_(True), torch.from_numpy(fq).to(dev)
    SP, SI, _ = sample_surface(Vq, Fq, n, seed=6)
    assert np.bincount(SI.cpu().numpy()).min() > 64
    save("sample_few_faces_P", SP), save("sample_few_faces_grad_V", grads((SP * weights(SP)).sum(), Vq)[0])

    VB = V2.clone().requires_grad_(True)
    ch = chamfer_distance(Vg, tf, VB, tf, 1 << 14, seed=4)
    gA, gB = grads(ch, Vg, VB)
    save("chamfer", ch), save("chamfer_grad_VA", gA), save("chamfer_grad_VB", gB)
    del ch, Sd, sqrD, t

    # ---- the remaining caller workspaces: the pairs of two icospheres that cross, the level set of a noisy ball with its gradient in
    # the field, the two mesh-geometry functions with their gradients
    from largesteps.distance import self_intersections
    from largesteps.levelset import isosurface
    from largesteps.meshops import average_edge_length, massmatrix_voronoi

    vx, fx = synthetic.icosphere(8)
    pairs = self_intersections(dev_f32(np.concatenate([vx, vx + np.array([0.7, 0.1, 0.05])])), torch.from_numpy(np.concatenate([fx, fx + vx.shape[0]])).to(dev))
    assert pairs.shape[0] > 64, "the two spheres must cross"
    save("selfx_pairs", pairs)
    ax = np.linspace(-1.0, 1.0, 24)
    ball = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.6 + 0.02 * rng.standard_normal((24, 24, 24))
    field = dev_f32(ball).requires_grad_(True)
    IV, IF, IE = isosurface(field, 0.0, (-1.0, -1.0, -1.0), 2.0 / 23.0, return_edges=True)
    assert IV.shape[0] > 0 and IF.shape[0] > 0
    save("iso_V", IV), save("iso_F", IF), save("iso_E", IE), save("iso_grad_S", grads((IV * weights(IV)).sum(), field)[0])
    mass, ael = massmatrix_voronoi(Vg, tf), average_edge_length(Vg, tf)
    save("meshgeom_mass", mass), save("meshgeom_mass_grad_V", grads((mass * weights(mass)).sum(), Vg)[0])
    save("meshgeom_edge_length", ael), save("meshgeom_edge_length_grad_V", grads(ael.sum(), Vg)[0])

    torch.cuda.synchronize()
    print(f"wrote {len(os.listdir(out))} files to {out} with {os.environ.get('LARGESTEPS_HIP_LIB', 'the package library')}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
