#!/usr/bin/env python3
"""
Golden fixtures for the vertex-normal row: EXECUTES the reference's scripts/geometry.py
(compute_face_normals :91-110, compute_vertex_normals :115-147) on CPU tensors in the dev container and records
outputs and autograd gradients.         python tests/golden/make_golden_normals.py
                                        python tests/golden/make_golden_normals.py --scale    (prints, writes nothing)
--scale measures, on the meshes of tests/normals_scale_cases.py, how far the reference's OWN fp32 arithmetic is from the fp64
statement (oracle/normals.py): the two tolerances of tests/test_normals_scale_gpu.py that are measured and not derived.

The file is pure torch (no device literals), so it is imported unmodified from /root/reference/scripts. The reference
cannot travel to the GPU box, hence the committed fixture tests/golden/reference_normals.npz.
Noteworthy reference behaviour that the fixture pins: `d0 / torch.norm(d0)` divides by the Frobenius norm of the WHOLE
(3, F) edge matrix, not per face -- the "angle" weights are acos(e_a . e_b / (||E_a||_F ||E_b||_F)).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "large-steps-pytorch_amd", "largesteps"))
import synthetic  # noqa: E402


def degenerate_meshes():
    """plane(6) plus one degenerate face each: three extra collinear vertices (zero area, three distinct vertices), and a face that
    names a vertex twice. The reference gives NaN in that face's normal, on its vertices' normals, and -- through the three global
    norms -- in every row of the gradients that pass through the vertex normals."""
    v, f = synthetic.plane(6)
    line = np.array([[2.0, 2.0, 1.0], [2.5, 2.25, 1.5], [3.0, 2.5, 2.0]], np.float32)
    V = v.shape[0]
    return {"degenerate_collinear": (np.concatenate([v, line]), np.concatenate([f, [[V, V + 1, V + 2]]])),
            "degenerate_repeated": (v, np.concatenate([f, [[7, 7, 8]]]))}


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_scripts_geometry", "/root/reference/scripts/geometry.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def scale():
    """The reference on the CPU (fp32 torch) against the fp64 statement, on the jittered planes of the scale test."""
    for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", ".."), os.path.join(HERE, "..", "..", "large-steps-pytorch_amd")):
        sys.path.insert(0, p)
    import normals_scale_cases as nc
    from oracle import normals as on
    ref = load_reference()
    for n in nc.SIZES:
        v, f = nc.jittered_plane(n)
        F, V = f.shape[0], v.shape[0]
        assert (F, V, nc.pair_G(F)) == nc.SIZES[n]
        fn64 = on.face_normals(v, f)
        N64 = on.edge_norms(v, f)
        tv, tf = torch.from_numpy(v), torch.from_numpy(f)
        e = [tv[tf[:, 1]] - tv[tf[:, 0]], tv[tf[:, 2]] - tv[tf[:, 0]], tv[tf[:, 2]] - tv[tf[:, 1]]]
        print(f"n = {n}: F = {F}, V = {V}; torch.norm fp32 of the edge matrices, relative to fp64:",
              " ".join(f"{abs(float(torch.norm(x.T)) - N) / N:.2e}" for x, N in zip(e, N64)))
        # 2b: the per-face terms of dL/dN formed in fp32 (sums in fp64) against fp64, on the inputs the test builds
        w = nc.tail_weights(n, V, f)
        if nc.tail_start(n) is not None:
            raw32, N32 = nc.tail_raw(n, V), N64.astype(np.float32)
            g_raw32 = on.normalize_rows_backward(raw32, w).astype(np.float32)
            g64 = on.norm_gradients(v, f, fn64, g_raw=g_raw32, norms=N32)
            g32 = on.norm_gradients(v, f, fn64, g_raw=g_raw32, norms=N32, dtype=np.float32)
            head = on.norm_gradients(v, f, fn64, g_raw=g_raw32, norms=N32, faces=(0, nc.tail_start(n)))
            print(f"    gN fp64 {g64}; per-face terms in fp32: max |gN32 - gN64| / max |gN64| = {np.abs(g32 - g64).max() / np.abs(g64).max():.3e};"
                  f" without the tail: |head - full| / max |gN64| = {np.abs(head - g64) / np.abs(g64).max()}")
        if n not in nc.END_TO_END:
            continue
        # 2c: the vertex gradient with the face normals held constant (angles and norms only)
        w = nc.plain_weights(n, V)
        tvg = tv.clone().requires_grad_(True)
        fn32 = ref.compute_face_normals(tvg, tf)
        vn = ref.compute_vertex_normals(tvg, tf, fn32)
        g_all, = torch.autograd.grad((vn * torch.from_numpy(w)).sum(), tvg)
        tv2 = tv.clone().requires_grad_(True)
        g_const, = torch.autograd.grad((ref.compute_vertex_normals(tv2, tf, fn32.detach()) * torch.from_numpy(w)).sum(), tv2)
        gv64, gfn64 = on.vertex_normals_backward(v, f, fn64, w)
        gall64 = gv64 + on.face_normals_backward(v, f, gfn64)
        vn64 = on.vertex_normals(v, f, fn64)
        print(f"    reference fp32 vs fp64: fn {np.abs(fn32.detach().numpy() - fn64).max():.2e}, vn {np.abs(vn.detach().numpy() - vn64).max():.2e},"
              f" g_all {np.abs(g_all.numpy() - gall64).max() / np.abs(gall64).max():.2e} of max |g64| = {np.abs(gall64).max():.3e};"
              f" fn constant: max |gv32 - gv64| / max |gv64| = {np.abs(g_const.numpy() - gv64).max() / np.abs(gv64).max():.3e}"
              f" (max |gv64| = {np.abs(gv64).max():.3e})")


def main():
    ref = load_reference()
    meshes = {
        "tetra": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)),
        "quad": (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int64)),
        "ico3": synthetic.icosphere(3),
        "ico8_noisy": (synthetic.perturb(synthetic.icosphere(8)[0], radial=0.05, tangential=0.2, edge=0.15, seed=3), synthetic.icosphere(8)[1]),
        "plane9": synthetic.plane(9),
        "unreferenced": (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int64)),
    }
    meshes.update(degenerate_meshes())           # appended: the arrays of the meshes above keep their random draws, bit for bit
    out = {}
    rng = np.random.default_rng(11)
    for name, (v, f) in meshes.items():
        tv = torch.from_numpy(v.astype(np.float32)).requires_grad_(True)
        tf = torch.from_numpy(f.astype(np.int64))
        fn = ref.compute_face_normals(tv, tf)                    # (3, F)
        vn = ref.compute_vertex_normals(tv, tf, fn)              # (V, 3)
        w_v = torch.from_numpy(rng.standard_normal(vn.shape).astype(np.float32))
        w_f = torch.from_numpy(rng.standard_normal(fn.shape).astype(np.float32))
        # gradient through both functions (what the optimisation loop back-propagates)
        g_all, = torch.autograd.grad((vn * w_v).sum() + 0.0 * fn.sum(), tv, retain_graph=True)
        # gradient of the face normals alone
        g_face, = torch.autograd.grad((fn * w_f).sum(), tv, retain_graph=True)
        # gradient of the vertex normals with the face normals treated as a constant input
        fn_c = fn.detach().requires_grad_(True)
        tv2 = tv.detach().clone().requires_grad_(True)
        vn2 = ref.compute_vertex_normals(tv2, tf, fn_c)
        g_v_only, g_fn = torch.autograd.grad((vn2 * w_v).sum(), (tv2, fn_c))
        out.update({f"{name}/verts": v.astype(np.float32), f"{name}/faces": f.astype(np.int64),
                    f"{name}/face_normals": fn.detach().numpy(), f"{name}/vertex_normals": vn.detach().numpy(),
                    f"{name}/w_v": w_v.numpy(), f"{name}/w_f": w_f.numpy(), f"{name}/grad_all": g_all.numpy(),
                    f"{name}/grad_face": g_face.numpy(), f"{name}/grad_vn_verts": g_v_only.numpy(), f"{name}/grad_vn_fn": g_fn.numpy()})
    np.savez_compressed(os.path.join(HERE, "reference_normals.npz"), **out)
    print("wrote", len(out), "arrays:", sorted({k.split('/')[0] for k in out}))


if __name__ == "__main__":
    scale() if "--scale" in sys.argv[1:] else main()
