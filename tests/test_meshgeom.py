"""
average_edge_length / massmatrix_voronoi (reference scripts/geometry.py:13-33, :35-89): the numpy statement
(tests/meshgeom_statement.py) vs the reference-generated fixture (CPU), the HIP kernels (csrc/meshgeom.hip) vs fixture and
statement (-m gpu). Fixture: tests/golden/reference_meshgeom.npz = outputs AND torch-autograd gradients of the reference's
own functions (tests/golden/make_golden_meshgeom.py).
"""
import inspect
import os

import numpy as np
import pytest
import torch

import meshgeom_statement as ms

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ["tetra", "quad", "obtuse_strip", "ico3", "ico8_noisy", "plane9", "unreferenced", "zero_edge", "collinear"]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "reference_meshgeom.npz"))


def close(a, b, atol):
    ok = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), ok), "NaN pattern differs from the reference"
    assert np.abs(a[ok] - b[ok]).max(initial=0.0) <= atol


def scale(a):
    a = a[np.isfinite(a)]
    return max(np.abs(a).max(initial=0.0), 1e-30)


# ---- CPU: the statement against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_statement_vs_reference(ref, name):
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    obtuse = ms.reference_obtuse(v, f)
    mass = ref[f"{name}/mass"]
    close(ms.massmatrix_voronoi(v, f, obtuse=obtuse), mass, 1e-6 * scale(mass))
    avg = float(ref[f"{name}/avg_edge"])
    assert abs(ms.average_edge_length(v, f) - avg) <= 1e-6 * avg
    g = ref[f"{name}/grad_mass"]
    close(ms.massmatrix_voronoi_backward(v, f, ref[f"{name}/w"], obtuse=obtuse), g, 2e-6 * scale(g))
    g = ref[f"{name}/grad_avg"]
    close(ms.average_edge_length_backward(v, f), g, 1e-6 * scale(g))


def test_fixture_covers_every_branch(ref):
    """the obtuse strip fires each torch.where override (corner k of face k), the special meshes show what they are for"""
    ob = ms.reference_obtuse(ref["obtuse_strip/verts"], ref["obtuse_strip/faces"])
    assert np.array_equal(ob, np.eye(3, dtype=bool))
    assert ref["unreferenced/mass"][4] == 0.0
    assert np.isnan(ref["zero_edge/mass"]).sum() == 3 and np.isfinite(ref["zero_edge/mass"][3:]).all()
    assert np.isfinite(ref["collinear/mass"]).all() and not np.isfinite(ref["collinear/grad_mass"]).all()
    # quad: the right angle's fp32 cosine is 0 (not obtuse) while the fp64 one is negative -- why the statement takes fp32 branches
    v, f = ref["quad/verts"], ref["quad/faces"]
    assert not np.array_equal(ms.reference_obtuse(v, f), ms.face_terms(v, f)["obtuse"])


def test_statement_gradients_are_derivatives():
    """central differences of the statement's own forward (fp64)"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(2)
    v = synthetic.perturb(v, radial=0.1, tangential=0.2, edge=0.5, seed=4).astype(np.float64)
    rng = np.random.default_rng(0)
    w = rng.standard_normal(v.shape[0])
    g = ms.massmatrix_voronoi_backward(v, f, w)
    ga = ms.average_edge_length_backward(v, f, 1.7)
    assert ms.face_terms(v, f)["obtuse"].any()
    for _ in range(4):
        d = rng.standard_normal(v.shape)
        h = 1e-6
        fd = ((ms.massmatrix_voronoi(v + h * d, f) * w).sum() - (ms.massmatrix_voronoi(v - h * d, f) * w).sum()) / (2 * h)
        assert abs(fd - (g * d).sum()) <= 1e-6 * max(1.0, abs(fd))
        fa = 1.7 * (ms.average_edge_length(v + h * d, f) - ms.average_edge_length(v - h * d, f)) / (2 * h)
        assert abs(fa - (ga * d).sum()) <= 1e-7 * max(1.0, abs(fa))


def test_public_signatures():
    from largesteps import meshops
    for fn in (meshops.average_edge_length, meshops.massmatrix_voronoi):
        assert list(inspect.signature(fn).parameters) == ["verts", "faces"]
        assert fn.__doc__
    with pytest.raises(RuntimeError):                        # no CPU path
        meshops.massmatrix_voronoi(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]))
    with pytest.raises(RuntimeError):
        meshops.average_edge_length(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]))


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ulp_close(a, b, n):
    ok = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), ok), "NaN pattern differs from the reference"
    assert (np.abs(a[ok] - b[ok]) <= n * np.spacing(np.abs(b[ok]).astype(np.float32))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_hip_vs_reference(ref, dev, name):
    from largesteps.meshops import average_edge_length, massmatrix_voronoi
    v, f = ref[f"{name}/verts"], ref[f"{name}/faces"]
    res = {}
    for idx in (np.int64, np.int32):
        tv = _t(v, dev).requires_grad_(True)
        tf = _t(f.astype(idx), dev)
        mass = massmatrix_voronoi(tv, tf)
        avg = average_edge_length(tv, tf)
        assert mass.shape == (v.shape[0],) and mass.dtype == torch.float32 and avg.shape == () and avg.dtype == torch.float32
        g_mass, = torch.autograd.grad((mass * _t(ref[f"{name}/w"], dev)).sum(), tv)
        g_avg, = torch.autograd.grad(avg, tv)
        res[idx] = [x.detach().cpu().numpy() for x in (mass, avg, g_mass, g_avg)]
    for a, b in zip(res[np.int64], res[np.int32]):           # int32 faces: the same bits
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    mass, avg, g_mass, g_avg = res[np.int64]
    ulp_close(mass, ref[f"{name}/mass"], 4)
    assert abs(float(avg) - float(ref[f"{name}/avg_edge"])) <= 1e-6 * abs(float(ref[f"{name}/avg_edge"]))
    close(g_mass, ref[f"{name}/grad_mass"], 1e-5 * scale(ref[f"{name}/grad_mass"]))
    close(g_avg, ref[f"{name}/grad_avg"], 1e-6 * scale(ref[f"{name}/grad_avg"]))


@pytest.mark.gpu
def test_hip_1m_vertices_vs_statement(dev):
    from largesteps import synthetic
    from largesteps.meshops import average_edge_length, massmatrix_voronoi
    v, f, _ = synthetic.config_mesh("cfg4b_sphere1m")
    tv, tf = _t(v, dev).requires_grad_(True), _t(f, dev)
    w = np.random.default_rng(0).standard_normal(v.shape[0]).astype(np.float32)
    tw = _t(w, dev)

    def run():
        mass = massmatrix_voronoi(tv, tf)
        avg = average_edge_length(tv, tf)
        g_mass, = torch.autograd.grad((mass * tw).sum(), tv)
        g_avg, = torch.autograd.grad(avg, tv)
        return [x.detach() for x in (mass, avg, g_mass, g_avg)]

    a, b = run(), run()
    for x, y in zip(a, b):                                   # no atomics: bitwise reproducible
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    mass, avg, g_mass, g_avg = (x.cpu().numpy() for x in a)
    # the forward is the reference's fp32 arithmetic: the fp32 statement in the same operation order within 4 ulp (bitwise in practice)
    obtuse = ms.reference_obtuse(v, f)
    ulp_close(mass, ms.massmatrix_voronoi(v, f, np.float32), 4)
    # against fp64, per vertex: relative to the vertex's value (forward) or to the sum of the magnitudes of the face contributions
    # that meet there (backward), times the cancellation factor of its worst face (Heron's formula and the barycentric sum lose
    # digits on needles; this mesh is full of them) -- the reference's own fp32 formulation stays below 3e-7 of this scale
    kap = ms.vertex_condition(v, f)[:, None]
    m64 = ms.massmatrix_voronoi(v, f, obtuse=obtuse)
    assert np.isfinite(m64).all() and (m64 > 0).all()
    assert (np.abs(mass - m64) <= 1e-5 * np.abs(m64) * kap[:, 0]).all()
    a64 = ms.average_edge_length(v, f)
    assert abs(float(avg) - a64) <= 1e-6 * a64
    g64, mag = ms.massmatrix_voronoi_backward(v, f, w, obtuse=obtuse, magnitude=True)
    assert (np.abs(g_mass - g64) <= 1e-5 * mag * kap).all()
    ga64, mag = ms.average_edge_length_backward(v, f, magnitude=True)
    assert (np.abs(g_avg - ga64) <= 1e-6 * mag).all()


def index_width_meshes(name):
    """the meshes of the same test of csrc/normals.hip (tests/test_normals.py). spike: a fan of 40 triangles around vertex 0 (valence 40
    exceeds the 4-corner request group) + an unreferenced vertex; cfg1_icosphere2k: 5120 faces; its cut: the last 7 faces dropped"""
    from largesteps import synthetic
    if name == "spike":
        k = 40
        ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
        v = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(3 * ang)], 1), [[5, 5, 5]]]).astype(np.float32)
        return v, np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], 1)
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
    point of csrc/meshgeom.hip through the C ABI with idx_bytes = 4 and 8 on the same mesh and the same corner ranking -- every output
    bit-equal."""
    from largesteps import _native, meshops, normals
    v, f = index_width_meshes(name)
    tv, f32 = _t(v.astype(np.float32), dev), _t(f.astype(np.int32), dev)
    vv, ff, vptr, cpos, order = normals._prep(tv, f32)
    assert ff.dtype == torch.int32
    F, V = ff.shape[0], vv.shape[0]
    lib, p = _native.lib(), _native.ptr
    gen = torch.Generator(device=dev).manual_seed(0)
    g_mass, g_avg = torch.randn(V, device=dev, generator=gen), torch.randn((), device=dev, generator=gen)

    def run(faces):
        mesh = (p(vv), p(faces), faces.element_size(), F, V)
        ws = meshops._workspace(F, V, dev)
        tail = (p(ws), ws.numel(), dev.index, _native.stream_of(dev))
        o = {"mass": torch.zeros(V, device=dev), "avg": torch.zeros((), device=dev), "g_mass": torch.zeros((V, 3), device=dev),
             "g_avg": torch.zeros((V, 3), device=dev)}
        _native.check(lib.ls_massmatrix_voronoi(*mesh, p(vptr), p(order), p(o["mass"]), *tail[2:]))
        _native.check(lib.ls_massmatrix_voronoi_backward(*mesh, p(vptr), p(cpos), p(g_mass), p(o["g_mass"]), *tail))
        _native.check(lib.ls_average_edge_length(*mesh, p(o["avg"]), *tail))
        _native.check(lib.ls_average_edge_length_backward(*mesh, p(vptr), p(cpos), p(g_avg), p(o["g_avg"]), *tail))
        torch.cuda.synchronize()
        return o

    narrow, wide = run(ff), run(ff.to(torch.int64))
    assert_same_bits({k: x.reshape(-1) for k, x in narrow.items()}, {k: x.reshape(-1) for k, x in wide.items()})
    assert bool((narrow["mass"] > 0).any()) and float(narrow["avg"]) > 0 and bool(narrow["g_mass"].abs().max() > 0)      # the kernels ran
    assert bool(narrow["mass"][-1] == 0) == (name == "spike")                                    # the unreferenced vertex


@pytest.mark.gpu
def test_hip_graph_capture_matches_eager(dev):
    from largesteps import synthetic
    from largesteps.capture import CapturedStep
    from largesteps.meshops import average_edge_length, massmatrix_voronoi
    v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    tv, tf = _t(v, dev).requires_grad_(True), _t(f.astype(np.int32), dev)
    tw = torch.randn(v.shape[0], device=dev)

    def body():
        mass = massmatrix_voronoi(tv, tf)
        avg = average_edge_length(tv, tf)
        g, = torch.autograd.grad((mass * tw).sum() + avg, tv)
        return mass.detach(), avg.detach(), g

    step = CapturedStep(body, warmup=2)
    with torch.no_grad():
        tv.add_(0.01 * torch.randn_like(tv))                 # replay reads the new positions in place
    got = [x.clone() for x in step()]
    want = body()
    for x, y in zip(got, want):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.gpu
def test_hip_through_from_differential(dev):
    """massmatrix_voronoi(from_differential(M, u)) back-propagates into u: against central differences of the fp64 statement composed
    with an fp64 solve of the same M"""
    from largesteps import synthetic
    from largesteps.geometry import compute_matrix
    from largesteps.meshops import massmatrix_voronoi
    from largesteps.parameterize import from_differential, to_differential
    v, f = synthetic.icosphere(3)
    v = synthetic.perturb(v, radial=0.05, tangential=0.1, edge=0.2, seed=2)
    tv, tf = _t(v, dev), _t(f, dev)
    M = compute_matrix(tv, tf, 10.0)
    u = to_differential(M, tv).detach().clone().requires_grad_(True)
    w = np.random.default_rng(3).standard_normal(v.shape[0])
    x = from_differential(M, u, "Cholesky")
    g_u, = torch.autograd.grad((massmatrix_voronoi(x, tf) * _t(w.astype(np.float32), dev)).sum(), u)
    g_u = g_u.cpu().numpy().astype(np.float64)
    M64 = M.to_dense().cpu().numpy().astype(np.float64)
    u64 = u.detach().cpu().numpy().astype(np.float64)

    def loss(uu):
        return float((ms.massmatrix_voronoi(np.linalg.solve(M64, uu), f) * w).sum())

    rng = np.random.default_rng(4)
    for _ in range(4):
        d = rng.standard_normal(u64.shape)
        h = 1e-5
        fd = (loss(u64 + h * d) - loss(u64 - h * d)) / (2 * h)
        assert abs(fd - (g_u * d).sum()) <= 1e-4 * max(abs(fd), np.abs(g_u).sum() * 1e-2)


@pytest.mark.gpu
def test_hip_errors_and_edge_cases(ref, dev):
    from largesteps.meshops import average_edge_length, massmatrix_voronoi
    v, f = ref["ico3/verts"], ref["ico3/faces"]
    tv, tf = _t(v, dev), _t(f, dev)
    bad = _t(np.array([[0, 1, v.shape[0]]]), dev)
    with pytest.raises(IndexError):
        massmatrix_voronoi(tv, bad)
    with pytest.raises(IndexError):
        average_edge_length(tv, bad)
    with pytest.raises(RuntimeError):
        massmatrix_voronoi(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(RuntimeError):
        average_edge_length(tv, torch.from_numpy(f))
    with pytest.raises(TypeError):
        massmatrix_voronoi(tv, tf.to(torch.int16))
    with pytest.raises(ValueError):
        average_edge_length(tv[:, :2], tf)
    # F == 0: the reference's 0 / 0 and an all-zero mass; the gradients are zero
    tv0 = tv.clone().requires_grad_(True)
    empty = torch.zeros((0, 3), dtype=torch.int64, device=dev)
    avg0, mass0 = average_edge_length(tv0, empty), massmatrix_voronoi(tv0, empty)
    assert torch.isnan(avg0).item() and torch.equal(mass0, torch.zeros_like(mass0))
    g0, = torch.autograd.grad(mass0.sum() + 0.0 * avg0.nan_to_num(), tv0)
    assert torch.equal(g0, torch.zeros_like(g0))
    # non-contiguous vertices: the values and gradients of the contiguous copy
    wide = torch.zeros((v.shape[0], 5), device=dev)
    wide[:, 1:4] = tv
    nc = wide[:, 1:4].requires_grad_(True)
    assert not nc.is_contiguous()
    tc = tv.clone().requires_grad_(True)
    tw = torch.randn(v.shape[0], device=dev)
    for fn in (massmatrix_voronoi, average_edge_length):
        a, b = fn(nc, tf), fn(tc, tf)
        assert torch.equal(a, b)
        ga, = torch.autograd.grad((a * (tw if a.dim() else 1.0)).sum(), nc)
        gb, = torch.autograd.grad((b * (tw if b.dim() else 1.0)).sum(), tc)
        assert torch.equal(ga, gb)
