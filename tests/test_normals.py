"""
Vertex / face normals: oracle vs the reference-generated fixture (CPU), HIP kernels vs
oracle and fixture (-m gpu). Fixture: tests/golden/reference_normals.npz = outputs AND torch-autograd gradients of the
reference's own scripts/geometry.py (tests/golden/make_golden_normals.py).
"""
import os

import numpy as np
import pytest
import torch

from oracle import normals as on

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ["tetra", "quad", "ico3", "ico8_noisy", "plane9", "unreferenced"]
# plane(6) plus one zero-area face (three collinear vertices / a vertex named twice): NaN in that face's normal, on its vertices'
# normals and, through the three global norms, in every row of the gradients behind the vertex normals -- close() compares the patterns
DEGENERATE = ["degenerate_collinear", "degenerate_repeated"]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "reference_normals.npz"))


def amax(x):
    """max |x| over the finite entries (the fixture's NaN entries are compared as a pattern, by close())"""
    return float(np.abs(x[np.isfinite(x)]).max(initial=0.0))


def close(a, b, atol):
    ok = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), ok), "NaN pattern differs from the reference"
    assert np.abs(a[ok] - b[ok]).max(initial=0.0) <= atol


@pytest.mark.parametrize("name", MESHES + DEGENERATE)
def test_oracle_vs_reference(ref, name):
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    fn = on.face_normals(v, f)
    close(fn, ref[f"{name}/face_normals"], 3e-7)
    close(on.vertex_normals(v, f, fn), ref[f"{name}/vertex_normals"], 3e-7)
    gscale = max(amax(ref[f"{name}/grad_all"]), 1e-3)
    close(on.face_normals_backward(v, f, ref[f"{name}/w_f"]), ref[f"{name}/grad_face"], 1e-6 * max(amax(ref[f"{name}/grad_face"]), 1.0))
    gv, gfn = on.vertex_normals_backward(v, f, ref[f"{name}/face_normals"].astype(np.float64), ref[f"{name}/w_v"])
    close(gv, ref[f"{name}/grad_vn_verts"], 2e-6 * gscale)
    close(gfn, ref[f"{name}/grad_vn_fn"], 1e-6 * max(amax(ref[f"{name}/grad_vn_fn"]), 1.0))
    close(gv + on.face_normals_backward(v, f, gfn), ref[f"{name}/grad_all"], 2e-6 * gscale)


def test_oracle_gradients_are_derivatives():
    """central differences of the oracle's own forward, incl. the global-norm terms"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(2)
    v = (v * (1.0 + 0.1 * np.random.default_rng(0).standard_normal((v.shape[0], 1)))).astype(np.float64)
    w = np.random.default_rng(1).standard_normal(v.shape)
    loss = lambda x: float((on.vertex_normals(x, f, on.face_normals(x, f)) * w).sum())    # noqa: E731
    fn = on.face_normals(v, f)
    gv, gfn = on.vertex_normals_backward(v, f, fn, w)
    g = gv + on.face_normals_backward(v, f, gfn)
    rng = np.random.default_rng(2)
    for _ in range(6):
        d = rng.standard_normal(v.shape)
        h = 1e-6
        fd = (loss(v + h * d) - loss(v - h * d)) / (2 * h)
        assert abs(fd - (g * d).sum()) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize("name", MESHES + DEGENERATE)
def test_statement_intermediates_vs_reference(ref, name):
    """the intermediate values the scale test compares device buffers with -- the three global norms, g_raw, the three gN sums, the
    per-face gradient of the face normals -- against the fixture, the older oracle functions and formulas written out here"""
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    fn, w = ref[f"{name}/face_normals"].astype(np.float64), ref[f"{name}/w_v"]
    v64 = v.astype(np.float64)
    gv, gfn, t = on.vertex_normals_backward(v, f, fn, w, return_terms=True)
    gv_b, gfn_b = on.vertex_normals_backward(v, f, fn, w)
    assert np.array_equal(gv, gv_b, equal_nan=True) and np.array_equal(gfn, gfn_b, equal_nan=True) and gfn is t["grad_fn"]
    # norms: torch.norm of the reference's (3, F) edge matrices
    edges = [v64[f[:, b]] - v64[f[:, a]] for a, b in ((0, 1), (0, 2), (1, 2))]
    assert np.allclose(t["norms"], [np.linalg.norm(e) for e in edges], rtol=1e-14, atol=0) and np.array_equal(t["norms"], on.edge_norms(v, f))
    out, raw = on.vertex_normals(v, f, fn, return_raw=True)
    assert np.array_equal(t["raw"], raw, equal_nan=True)
    close(out, ref[f"{name}/vertex_normals"], 3e-7)
    # g_raw: the derivative of sum(w * raw / |raw|) w.r.t. raw, row by row: (I - o o^T) w / |raw|
    R = np.linalg.norm(raw, axis=1)
    ok = np.isfinite(R) & (R > 0)
    assert np.array_equal(np.isfinite(t["g_raw"]).all(axis=1), ok)
    for r in np.flatnonzero(ok):
        o = raw[r] / R[r]
        assert np.abs(t["g_raw"][r] - (np.eye(3) - np.outer(o, o)) @ w[r] / R[r]).max() <= 1e-12 * np.abs(w[r]).max() / R[r]
    # per-face gradient of the face normals: sum over the corners of theta_i g_raw[f_i] = what the reference's autograd gives
    close(t["grad_fn"], ref[f"{name}/grad_vn_fn"], 1e-6 * max(amax(ref[f"{name}/grad_vn_fn"]), 1.0))
    # gN: one value per norm; over a face range; from given raw / g_raw / norms
    F = f.shape[0]
    gN = on.norm_gradients(v, f, fn, g=w)
    assert gN.shape == (3,) and np.array_equal(gN, t["gN"], equal_nan=True)
    if name in DEGENERATE:
        assert np.isnan(gN).all() and np.isnan(gv).all()       # the NaN of one face reaches every vertex through the norms
        return
    k = F // 3 + 1
    parts = on.norm_gradients(v, f, fn, g=w, faces=(0, k)) + on.norm_gradients(v, f, fn, g=w, faces=(k, F))
    assert np.abs(parts - gN).max() <= 1e-13 * max(np.abs(gN).max(), 1e-300)
    assert np.array_equal(on.norm_gradients(v, f, fn, g=w, raw=raw), gN)
    assert np.array_equal(on.norm_gradients(v, f, fn, g_raw=t["g_raw"], norms=t["norms"]), gN)
    # given norms are used as given: the sum written out corner by corner, at the mesh's norms and at others
    def by_hand(N):
        out = np.zeros(3)
        for face, n_f in zip(f, fn.T):
            p = v64[face]
            for i, (na, nb) in enumerate(((0, 1), (2, 0), (1, 2))):
                s_ = np.dot(p[(i + 1) % 3] - p[i], p[(i + 2) % 3] - p[i]) / (N[na] * N[nb])
                gs = -np.dot(n_f, t["g_raw"][face[i]]) / np.sqrt(1.0 - s_ * s_) if abs(s_) < 1 else 0.0
                out[na] -= gs * s_ / N[na]
                out[nb] -= gs * s_ / N[nb]
        return out
    for N in (t["norms"], t["norms"] * np.array([2.0, 0.5, 3.0])):
        assert np.allclose(on.norm_gradients(v, f, fn, g_raw=t["g_raw"], norms=N), by_hand(N), rtol=1e-11, atol=1e-15 * np.abs(gN).max())
    # the reference's vertex gradient = the part through the corner angles with the norms held fixed + gN through dN/de = e / N
    gscale = max(amax(ref[f"{name}/grad_all"]), 1e-3)
    ct = on.corner_terms(v, f, fn, t["g_raw"])
    angle = np.zeros_like(v64)
    for i in range(3):
        ea, eb = v64[f[:, (i + 1) % 3]] - v64[f[:, i]], v64[f[:, (i + 2) % 3]] - v64[f[:, i]]
        na, nb = ((0, 1), (2, 0), (1, 2))[i]
        c = ct["gs"][i][:, None] / (t["norms"][na] * t["norms"][nb])
        for col, val in (((i + 1) % 3, c * eb), ((i + 2) % 3, c * ea), (i, -c * (ea + eb))):
            np.add.at(angle, f[:, col], val)
    through_norms = np.zeros_like(v64)
    for e, (a, b), g_, N in zip(edges, ((0, 1), (0, 2), (1, 2)), gN, t["norms"]):
        np.add.at(through_norms, f[:, b], g_ * e / N)
        np.add.at(through_norms, f[:, a], -g_ * e / N)
    close(angle + through_norms, ref[f"{name}/grad_vn_verts"], 2e-6 * gscale)
    # fp32 terms (the scale test's measure of the rounding floor) are the same statement, a few fp32 ulp away
    g32 = on.norm_gradients(v, f, fn, g_raw=t["g_raw"], norms=t["norms"], dtype=np.float32)
    mag = np.abs(ct["gN"]).sum(axis=1).max()
    assert g32.dtype == np.float64 and np.abs(g32 - gN).max() <= 32 * 2.0 ** -24 * mag


def test_statement_norm_gradients_are_derivatives():
    """central differences of the oracle's forward in the three global norms, taken as free variables (everything else fixed)"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(2)
    v = (v * (1.0 + 0.1 * np.random.default_rng(0).standard_normal((v.shape[0], 1)))).astype(np.float64)
    w = np.random.default_rng(1).standard_normal(v.shape)
    fn = on.face_normals(v, f)
    N = on.edge_norms(v, f)
    loss = lambda n: float((on.vertex_normals(v, f, fn, norms=n) * w).sum())    # noqa: E731
    assert loss(N) == float((on.vertex_normals(v, f, fn) * w).sum())
    gN = on.norm_gradients(v, f, fn, g=w)
    assert np.abs(gN).min() > 0
    for j in range(3):
        h = 1e-6 * N[j]
        d = np.zeros(3)
        d[j] = h
        fd = (loss(N + d) - loss(N - d)) / (2 * h)
        assert abs(fd - gN[j]) <= 1e-6 * max(1.0, abs(fd)), (j, fd, gN[j])
        assert abs(fd - gN[j]) <= 1e-5 * np.abs(gN).max(), (j, fd, gN[j])     # (relative to gN itself: |gN| << 1)
    # ... and the sum over a face range takes the forward (raw, norms) of the WHOLE mesh
    F = f.shape[0]
    assert np.allclose(on.norm_gradients(v, f, fn, g=w, faces=(0, 100)) + on.norm_gradients(v, f, fn, g=w, faces=(100, F)), gN, rtol=1e-12, atol=0)


def test_scale_meshes_cross_the_compiled_thresholds():
    """tests/test_normals_scale_gpu.py chooses its three meshes as the smallest that cross thresholds set by constants of csrc/: they
    are read from the sources that are compiled (tests/normals_scale_cases.py), and a change of PF, FIN, FIN_U, BLOCK or MESH_MAXG --
    or of how the launches use them -- fails here instead of leaving the second pass / slot / trip silently untested"""
    import sys
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import normals_scale_cases as nc
    assert (nc.BLOCK, nc.MESH_MAXG, nc.PF, nc.FIN, nc.FIN_U) == (256, 1024, 4, 1024, 4)
    for name, lines in nc.USES.items():
        src = nc.source(name)
        for line in lines:
            assert line in src, f"csrc/{name} no longer has `{line}`: the formulas of normals_scale_cases.py stand for it"
    # general path: plane(364) leaves 1,394 faces to a second pass of the capped grid, plane(363) none
    assert nc.SIZES[364][0] - nc.GENERAL_SWEEP == 1394 and 2 * 362 ** 2 <= nc.GENERAL_SWEEP
    # pair path: G just past one slot of k_finish3's threads (n = 726) and just past one trip of its loop (n = 1450)
    for n, slots in ((726, nc.FIN), (1450, nc.FIN * nc.FIN_U)):
        F, V, G = nc.SIZES[n]
        assert (F, V) == (2 * (n - 1) ** 2, n * n) and nc.pair_G(F) == G
        assert G > slots >= nc.pair_G(2 * (n - 2) ** 2) and nc.tail_start(n) == slots * nc.PAIR_FACES < F
    assert [nc.SIZES[n][2] for n in (364, 726, 1450)] == [258, 1027, 4101] and nc.tail_start(364) is None
    assert nc.FIN < 1027 <= 2 * nc.FIN and nc.FIN * nc.FIN_U < 4101 <= 2 * nc.FIN * nc.FIN_U


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [np.int64, np.int32])
@pytest.mark.parametrize("name", MESHES + DEGENERATE)
def test_hip_vs_reference(ref, dev, name, idx):
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"].astype(idx)
    tv = _t(v, dev).requires_grad_(True)
    tf = _t(f, dev)
    fn = compute_face_normals(tv, tf)
    vn = compute_vertex_normals(tv, tf, fn)
    assert fn.shape == (3, f.shape[0]) and vn.shape == v.shape and fn.dtype == torch.float32
    # fp32 kernels vs the reference's fp32 torch ops: a few ulp (different summation order in the scatter / norms)
    close(fn.detach().cpu().numpy(), ref[f"{name}/face_normals"], 1e-6)
    close(vn.detach().cpu().numpy(), ref[f"{name}/vertex_normals"], 2e-6)
    gscale = max(amax(ref[f"{name}/grad_all"]), 1e-3)
    g_all, = torch.autograd.grad((vn * _t(ref[f"{name}/w_v"], dev)).sum(), tv, retain_graph=True)
    close(g_all.cpu().numpy(), ref[f"{name}/grad_all"], 2e-5 * gscale)
    g_face, = torch.autograd.grad((fn * _t(ref[f"{name}/w_f"], dev)).sum(), tv, retain_graph=True)
    close(g_face.cpu().numpy(), ref[f"{name}/grad_face"], 1e-5 * max(amax(ref[f"{name}/grad_face"]), 1.0))
    # face normals as an independent input (the reference's signature allows it)
    fn_c = _t(ref[f"{name}/face_normals"], dev).requires_grad_(True)
    tv2 = _t(v, dev).requires_grad_(True)
    vn2 = compute_vertex_normals(tv2, tf, fn_c)
    gv, gfn = torch.autograd.grad((vn2 * _t(ref[f"{name}/w_v"], dev)).sum(), (tv2, fn_c))
    close(gv.cpu().numpy(), ref[f"{name}/grad_vn_verts"], 2e-5 * gscale)
    close(gfn.cpu().numpy(), ref[f"{name}/grad_vn_fn"], 1e-5 * max(amax(ref[f"{name}/grad_vn_fn"]), 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES + DEGENERATE)
def test_hip_pair_paths_vs_reference(ref, dev, name, monkeypatch):
    """compute_face_normals -> compute_vertex_normals on one mesh share passes (one corner buffer in the backward, the
    vertex gradient finished by the face-normal node). Every way the two nodes can meet in a backward call must give the
    reference's gradients: both outputs used, a backward that stops at the face normals followed by one that does not, two
    vertex-normal nodes on one face-normal tensor, and the general path (LARGESTEPS_NORMALS_PAIR=0) next to the pair."""
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    tv, tf = _t(v, dev).requires_grad_(True), _t(f, dev)
    w_v, w_f = _t(ref[f"{name}/w_v"], dev), _t(ref[f"{name}/w_f"], dev)
    g_all, g_face = ref[f"{name}/grad_all"], ref[f"{name}/grad_face"]
    tol = 2e-5 * max(amax(g_all), 1e-3) + 1e-5 * max(amax(g_face), 1.0)
    fn = compute_face_normals(tv, tf)
    vn = compute_vertex_normals(tv, tf, fn)
    assert getattr(fn, "_largesteps_pair", None) is not None
    both, = torch.autograd.grad((vn * w_v).sum() + (fn * w_f).sum(), tv, retain_graph=True)
    close(both.cpu().numpy(), g_all + g_face, tol)
    # a backward that ends at the face normals leaves nothing behind for the next one
    g_fn, = torch.autograd.grad((vn * w_v).sum(), fn, retain_graph=True)
    close(g_fn.cpu().numpy(), ref[f"{name}/grad_vn_fn"], 1e-5 * max(amax(ref[f"{name}/grad_vn_fn"]), 1.0))
    only_face, = torch.autograd.grad((fn * w_f).sum(), tv, retain_graph=True)
    close(only_face.cpu().numpy(), g_face, 1e-5 * max(amax(g_face), 1.0))
    # two vertex-normal nodes on the same face normals
    vn_b = compute_vertex_normals(tv, tf, fn)
    twice, = torch.autograd.grad((vn * w_v).sum() + (vn_b * w_v).sum(), tv, retain_graph=True)
    close(twice.cpu().numpy(), 2 * g_all, 2 * tol)
    # the pair and the general path agree (values: the same arithmetic; gradients: a different order of a few additions)
    g_pair, = torch.autograd.grad((vn * w_v).sum(), tv)
    monkeypatch.setenv("LARGESTEPS_NORMALS_PAIR", "0")
    fn2 = compute_face_normals(tv, tf)
    vn2 = compute_vertex_normals(tv, tf, fn2)
    assert torch.equal(fn2.view(torch.int32), fn.view(torch.int32))         # (bits: the NaN column of a degenerate face included)
    close(vn2.detach().cpu().numpy(), vn.detach().cpu().numpy(), 1e-6)
    g_gen, = torch.autograd.grad((vn2 * w_v).sum(), tv)
    close(g_gen.cpu().numpy(), g_all, tol)
    close(g_pair.cpu().numpy(), g_all, tol)
    # face normals computed without a graph: a constant for the vertex normals, in the pair's kernels as well
    monkeypatch.delenv("LARGESTEPS_NORMALS_PAIR")
    with torch.no_grad():
        fn3 = compute_face_normals(tv, tf)
    g_const, = torch.autograd.grad((compute_vertex_normals(tv, tf, fn3) * w_v).sum(), tv)
    close(g_const.cpu().numpy(), ref[f"{name}/grad_vn_verts"], 2e-5 * max(amax(g_all), 1e-3))
    # ... and switched to requires_grad afterwards: the tensor still carries the tag (same object, same version) but NO face-normal node
    # will run in the backward -- the vertex-normal node must finish the vertices' gradient itself (advisor's finding, round 3: the
    # hand-over was dropped and the gradient came back None)
    fn3.requires_grad_(True)
    assert fn3.grad_fn is None and getattr(fn3, "_largesteps_pair", None) is not None
    g_v, g_f = torch.autograd.grad((compute_vertex_normals(tv, tf, fn3) * w_v).sum(), (tv, fn3))
    close(g_v.cpu().numpy(), ref[f"{name}/grad_vn_verts"], 2e-5 * max(amax(g_all), 1e-3))
    close(g_f.cpu().numpy(), ref[f"{name}/grad_vn_fn"], 1e-5 * max(amax(ref[f"{name}/grad_vn_fn"]), 1.0))


def _spike(k=40):
    """a fan of k triangles around vertex 0 + an unreferenced vertex"""
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    v = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(3 * ang)], 1), [[5, 5, 5]]]).astype(np.float32)
    f = np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], 1)
    return v, f


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [np.int64, np.int32])
@pytest.mark.parametrize("name", MESHES + ["cfg2_bunny70k", "spike"])
def test_vertex_major_forward_equals_the_corner_buffer_forward(ref, dev, name, idx):
    """ls_vertex_normals_gathered (a thread per vertex recomputes the contributions of its corners in rank order; what the pair's forward
    runs) against ls_vertex_normals_from_norms (corner buffer written per face, summed per vertex), both through the C ABI on the same
    norms: the same bits in `raw` and `out`, NaN rows of unreferenced vertices included; a vertex of valence 40 walks its corners in
    several trips."""
    import ctypes
    from largesteps import _native, normals, synthetic
    if name == "spike":
        v, f = _spike()
    elif name.startswith("cfg"):
        v, f, _ = synthetic.config_mesh(name)
    else:
        v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    tv, tf = _t(v.astype(np.float32), dev), _t(f.astype(idx), dev)
    vv, ff, vptr, vcorner, order = normals._prep(tv, tf)
    assert torch.equal(order[vcorner.long()].cpu(), torch.arange(3 * f.shape[0], dtype=torch.int32))
    F, V = ff.shape[0], vv.shape[0]
    lib = _native.lib()
    ws = normals._workspace(F, V, dev)
    fn = torch.empty((3, F), device=dev)
    norms = torch.empty(3, device=dev)
    _native.check(lib.ls_face_normals_with_norms(_native.ptr(vv), _native.ptr(ff), ff.element_size(), F, V, _native.ptr(fn), _native.ptr(norms),
                                                 _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))
    out_a, raw_a, out_b, raw_b = (torch.empty_like(vv) for _ in range(4))
    _native.check(lib.ls_vertex_normals_from_norms(_native.ptr(vv), _native.ptr(ff), ff.element_size(), F, V, _native.ptr(vptr), _native.ptr(vcorner),
                                                   _native.ptr(norms), _native.ptr(out_a), _native.ptr(raw_a), _native.ptr(ws), ws.numel(),
                                                   dev.index, _native.stream_of(dev)))
    _native.check(lib.ls_vertex_normals_gathered(_native.ptr(vv), _native.ptr(ff), ff.element_size(), F, V, _native.ptr(vptr), _native.ptr(order),
                                                 _native.ptr(norms), _native.ptr(out_b), _native.ptr(raw_b), dev.index, _native.stream_of(dev)))
    torch.cuda.synchronize()
    for a, b in ((raw_a, raw_b), (out_a, out_b)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert lib.ls_vertex_normals_gathered(_native.ptr(vv), _native.ptr(ff), ff.element_size(), F, V, _native.ptr(vptr), None, _native.ptr(norms),
                                          _native.ptr(out_b), _native.ptr(raw_b), dev.index, _native.stream_of(dev)) == _native.LS_E_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "general"])
def test_hip_spike_vs_oracle(dev, pair, monkeypatch):
    """a vertex of valence 40 -- past the 8 corners k_gather_corners requests together and the 6 of the vertex-major forward -- against
    the fp64 oracle (test_vertex_major_forward_equals_the_corner_buffer_forward compares device paths only): forward and the three
    gradients at test_hip_vs_reference's tolerances, the NaN rows of the unreferenced vertex included"""
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    if not pair:
        monkeypatch.setenv("LARGESTEPS_NORMALS_PAIR", "0")
    v, f = _spike()
    rng = np.random.default_rng(4)
    w_v, w_f = rng.standard_normal(v.shape).astype(np.float32), rng.standard_normal((3, f.shape[0])).astype(np.float32)
    fn64 = on.face_normals(v, f)
    vn64 = on.vertex_normals(v, f, fn64)
    gv64, gfn64 = on.vertex_normals_backward(v, f, fn64, w_v)
    g_all64, g_face64 = gv64 + on.face_normals_backward(v, f, gfn64), on.face_normals_backward(v, f, w_f)
    assert np.isnan(vn64[-1]).all() and np.isfinite(vn64[:-1]).all() and np.bincount(f.ravel())[0] == 40
    tv, tf = _t(v, dev).requires_grad_(True), _t(f, dev)
    fn = compute_face_normals(tv, tf)
    vn = compute_vertex_normals(tv, tf, fn)
    close(fn.detach().cpu().numpy(), fn64, 1e-6)
    close(vn.detach().cpu().numpy(), vn64, 2e-6)
    gscale = max(amax(g_all64), 1e-3)
    g_all, = torch.autograd.grad((vn * _t(w_v, dev)).sum(), tv, retain_graph=True)
    close(g_all.cpu().numpy(), g_all64, 2e-5 * gscale)
    g_face, = torch.autograd.grad((fn * _t(w_f, dev)).sum(), tv, retain_graph=True)
    close(g_face.cpu().numpy(), g_face64, 1e-5 * max(amax(g_face64), 1.0))
    # face normals as a leaf: on the pair path the tagged tensor itself (no face-normal node), otherwise a copy
    with torch.no_grad():
        fn_c = compute_face_normals(tv, tf)
    fn_c.requires_grad_(True)
    gv, gfn = torch.autograd.grad((compute_vertex_normals(tv, tf, fn_c) * _t(w_v, dev)).sum(), (tv, fn_c))
    close(gv.cpu().numpy(), gv64, 2e-5 * gscale)
    close(gfn.cpu().numpy(), gfn64, 1e-5 * max(amax(gfn64), 1.0))


def index_width_meshes(name):
    """spike: valence 40 exceeds the 8- and 4-corner request groups, 40 faces leave the 4-faces-per-thread kernels a clamped tail;
    cfg1_icosphere2k: 5120 faces, several workgroups feed the fixed-order reductions (5120 = 5 x 1024: no tail there); its cut (the
    last 7 faces dropped) has both at once"""
    from largesteps import synthetic
    if name == "spike":
        return _spike()
    v, f, _ = synthetic.config_mesh("cfg1_icosphere2k")
    return v, (f[:-7] if name.endswith("_cut") else f)


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spike", "cfg1_icosphere2k", "cfg1_icosphere2k_cut"])
def test_int64_index_kernels_give_the_bits_of_the_int32_ones(dev, name):
    """The package narrows int64 faces to int32 (normals._prep), so nothing else runs the IDX = int64_t instantiations: every entry
    point of csrc/normals.hip through the C ABI with idx_bytes = 4 and 8 on the same mesh and the same corner ranking -- every output
    bit-equal, the NaN rows of the unreferenced vertex included."""
    from largesteps import _native, normals
    v, f = index_width_meshes(name)
    tv, f32 = _t(v.astype(np.float32), dev), _t(f.astype(np.int32), dev)
    vv, ff, vptr, cpos, order = normals._prep(tv, f32)
    assert ff.dtype == torch.int32
    F, V = ff.shape[0], vv.shape[0]
    lib, p = _native.lib(), _native.ptr
    gen = torch.Generator(device=dev).manual_seed(0)
    g_fn, g_out = torch.randn((3, F), device=dev, generator=gen), torch.randn((V, 3), device=dev, generator=gen)

    def run(faces):
        mesh = (p(vv), p(faces), faces.element_size(), F, V)
        ws = normals._workspace(F, V, dev)
        tail = (p(ws), ws.numel(), dev.index, _native.stream_of(dev))
        o = {k: torch.zeros((3, F), device=dev) for k in ("fn", "fn_w", "gfn", "pair_gfn")}
        o.update({k: torch.zeros((V, 3), device=dev) for k in ("fn_gv", "out", "raw", "gv", "out_n", "raw_n", "out_g", "raw_g", "g_raw", "pair_gv")})
        o.update({k: torch.zeros(4, device=dev) for k in ("norms", "norms_w", "gN")})
        _native.check(lib.ls_face_normals(*mesh, p(o["fn"]), *tail[2:]))
        _native.check(lib.ls_face_normals_backward(*mesh, p(vptr), p(cpos), p(g_fn), p(o["fn_gv"]), *tail))
        _native.check(lib.ls_vertex_normals(*mesh, p(vptr), p(cpos), p(o["fn"]), p(o["out"]), p(o["raw"]), p(o["norms"]), *tail))
        _native.check(lib.ls_vertex_normals_backward(*mesh, p(vptr), p(cpos), p(o["fn"]), p(o["raw"]), p(o["norms"]), p(g_out), p(o["gv"]),
                                                     p(o["gfn"]), *tail))
        _native.check(lib.ls_face_normals_with_norms(*mesh, p(o["fn_w"]), p(o["norms_w"]), *tail))
        _native.check(lib.ls_vertex_normals_from_norms(*mesh, p(vptr), p(cpos), p(o["norms_w"]), p(o["out_n"]), p(o["raw_n"]), *tail))
        _native.check(lib.ls_vertex_normals_gathered(*mesh, p(vptr), p(order), p(o["norms_w"]), p(o["out_g"]), p(o["raw_g"]), *tail[2:]))
        _native.check(lib.ls_normals_pair_backward_faces(*mesh, p(o["raw_n"]), p(o["norms_w"]), p(g_out), p(o["g_raw"]), p(o["gN"]),
                                                         p(o["pair_gfn"]), *tail))
        _native.check(lib.ls_normals_pair_backward_verts(*mesh, p(vptr), p(cpos), p(o["norms_w"]), p(o["g_raw"]), p(o["gN"]), p(g_fn),
                                                         p(o["pair_gv"]), *tail))
        torch.cuda.synchronize()
        return o

    narrow, wide = run(ff), run(ff.to(torch.int64))
    assert_same_bits(narrow, wide)
    assert torch.isfinite(narrow["fn"]).all() and bool(narrow["pair_gv"].abs().max() > 0)      # the kernels ran
    assert torch.isnan(narrow["out"]).any() == (name == "spike")


@pytest.mark.gpu
def test_hip_large_mesh_vs_oracle_and_errors(dev):
    from largesteps import synthetic
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    tv, tf = _t(v, dev).requires_grad_(True), _t(f, dev)
    fn = compute_face_normals(tv, tf)
    vn = compute_vertex_normals(tv, tf, fn)
    fn64 = on.face_normals(v, f)
    vn64 = on.vertex_normals(v, f, fn64)
    assert np.abs(fn.detach().cpu().numpy() - fn64).max() <= 2e-6
    assert np.abs(vn.detach().cpu().numpy() - vn64).max() <= 5e-6
    w = np.random.default_rng(0).standard_normal(v.shape).astype(np.float32)
    g, = torch.autograd.grad((vn * _t(w, dev)).sum(), tv)
    gv, gfn = on.vertex_normals_backward(v, f, fn64, w)
    g64 = gv + on.face_normals_backward(v, f, gfn)
    assert np.abs(g.cpu().numpy() - g64).max() <= 2e-4 * np.abs(g64).max()
    # no atomics anywhere: forward and backward are bitwise reproducible
    vn_b = compute_vertex_normals(tv, tf, compute_face_normals(tv, tf))
    g_b, = torch.autograd.grad((vn_b * _t(w, dev)).sum(), tv)
    assert torch.equal(vn_b, vn) and torch.equal(g_b, g)
    # size-independent property: unit length wherever a vertex is referenced
    assert float((vn.detach().norm(dim=1) - 1).abs().max()) <= 1e-5
    with pytest.raises(IndexError):
        compute_face_normals(tv, _t(np.array([[0, 1, v.shape[0]]]), dev))
    with pytest.raises(RuntimeError):
        compute_face_normals(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        compute_vertex_normals(tv, tf, fn[:, :-1])
    with pytest.raises(TypeError):
        compute_face_normals(tv, tf.to(torch.int16))


@pytest.mark.gpu
def test_plan_cache_is_tied_to_the_face_tensor():
    """Two different connectivities of identical shape, the first freed before the second is created (the caching allocator
    hands the second the same address): the corner ranking must be rebuilt, not reused."""
    import gc
    import torch
    from largesteps import synthetic
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    from oracle import normals as on
    dev = torch.device("cuda:0")
    v, f = synthetic.icosphere(6)
    rng = np.random.default_rng(0)
    tv = torch.from_numpy(v).to(dev)
    outs = []
    for trial in range(3):
        fp = f[rng.permutation(f.shape[0])][:, rng.permutation(3)] if trial else f
        # keep the orientation: a cyclic shift only
        fp = np.roll(f[rng.permutation(f.shape[0])], trial, axis=1)
        tf = torch.from_numpy(fp).to(dev)
        n = compute_vertex_normals(tv, tf, compute_face_normals(tv, tf)).cpu().numpy()
        ref = on.vertex_normals(v.astype(np.float64), fp, on.face_normals(v.astype(np.float64), fp))
        assert np.abs(n - ref).max() <= 1e-5
        outs.append(tf.data_ptr())
        del tf
        gc.collect()
