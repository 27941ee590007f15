"""
The ray query of largesteps.raycast without a device: the rule of tests/ray_statement.py on hand-worked cases (binary-fraction
coordinates, so every expected number is exact), its gradient against torch autograd of the closed form, the watertightness that the
rule promises, and the public surface with the argument errors that are raised before any device work.
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import ray_statement as rs
from largesteps import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = np.inf

TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F32)
TRI_F = np.array([[0, 1, 2]])


def one(o, d, v=TRI_V, f=TRI_F, trange=None):
    t, I, W = rs.closest(np.array([o], dtype=F32), np.array([d], dtype=F32), v, f, None if trange is None else np.array([trange], dtype=np.float64))
    hit = rs.any_hit(np.array([o], dtype=F32), np.array([d], dtype=F32), v, f, None if trange is None else np.array([trange], dtype=np.float64))
    assert bool(hit[0]) == (I[0] >= 0)
    return float(t[0]), int(I[0]), W[0].tolist()


MISS = (INF, -1, [0.0, 0.0, 0.0])


def test_a_centre_hit_with_its_t_and_weights():
    # (0.25, 0.25) = 0.5 a + 0.25 b + 0.25 c, from one unit above
    assert one([0.25, 0.25, 1], [0, 0, -1]) == (1.0, 0, [0.5, 0.25, 0.25])
    assert one([0.25, 0.25, 1], [0, 0, -2]) == (0.5, 0, [0.5, 0.25, 0.25])             # t is in units of |d|
    assert one([0.25, 0.25, -2], [0, 0, 1]) == (2.0, 0, [0.5, 0.25, 0.25])             # from the back: both orientations count
    # along another dominant axis: the triangle in the plane x = 0.5, the ray along +x from x = -1.5
    v = np.array([[0.5, 0, 0], [0.5, 1, 0], [0.5, 0, 1]], dtype=F32)
    assert one([-1.5, 0.5, 0.25], [4, 0, 0], v) == (0.5, 0, [0.25, 0.5, 0.25])
    # an oblique ray: from (0.25, 0.25, 1) + (0.5, 0.25, 0) towards (0.25, 0.25, 0)
    assert one([0.75, 0.5, 1], [-0.5, -0.25, -1]) == (1.0, 0, [0.5, 0.25, 0.25])


def grid(n=4, h=1.0 / 16):
    """(n + 1)^2 vertices h apart in the plane z = 0, two faces per cell split along the same diagonal: an interior vertex has 6 faces"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * h, j * h, np.zeros_like(i, dtype=np.float64)], -1).reshape(-1, 3).astype(F32)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    b, c, d = a + (n + 1), a + (n + 2), a + 1
    return v, np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 1).reshape(-1, 3)


def test_rays_through_a_shared_edge_and_a_shared_vertex_go_to_the_lowest_face():
    v, f = grid()
    # the interior vertex (2, 2): an edge function is exactly 0 in each of its six faces; all tie at t = 1
    k = 2 * 5 + 2
    around = np.nonzero((f == k).any(1))[0]
    assert around.size == 6
    o, d = np.array([[2 / 16, 2 / 16, 1]], dtype=F32), np.array([[0, 0, -1]], dtype=F32)
    hit, t, U, V, W, det = rs.faces_of_rays(o, d, v, f)
    assert np.array_equal(np.nonzero(hit[0])[0], around) and (t[0, around] == 1.0).all()
    assert ((U[0, around] == 0) | (V[0, around] == 0) | (W[0, around] == 0)).all()
    t1, I1, W1 = one(o[0], d[0], v, f)
    assert (t1, I1) == (1.0, int(around.min())) and sorted(W1) == [0.0, 0.0, 1.0]
    # the midpoint of the edge from vertex (2, 2) to (3, 2): two faces
    edge = np.nonzero((f == k).any(1) & (f == k + 5).any(1))[0]
    assert edge.size == 2
    o = np.array([[2 / 16 + 1 / 32, 2 / 16, 1]], dtype=F32)
    hit, t, *_ = rs.faces_of_rays(o, d, v, f)
    assert np.array_equal(np.nonzero(hit[0])[0], edge) and (t[0, edge] == 1.0).all()
    t2, I2, W2 = one(o[0], d[0], v, f)
    assert (t2, I2) == (1.0, int(edge.min())) and sorted(W2) == [0.0, 0.5, 0.5]
    # a boundary vertex and a boundary edge are hit too
    assert one([0, 0, 1], [0, 0, -1], v, f)[:2] == (1.0, 0)
    assert one([1 / 32, 0, 1], [0, 0, -1], v, f)[0] == 1.0


def test_parallel_rays_and_hits_behind_the_origin():
    assert one([-1, 0.25, 0.5], [1, 0, 0]) == MISS                     # parallel, above the plane
    assert one([-1, 0.25, 0.0], [1, 0, 0]) == MISS                     # in the plane: the sheared triangle has no area
    assert one([0.25, 0.25, 1], [0, 0, 1]) == MISS                     # the plane is behind: t = -1 < tmin = 0
    assert one([0.25, 0.25, 1], [0, 0, 1], trange=(-2.0, 0.0)) == (-1.0, 0, [0.5, 0.25, 0.25])
    assert one([2, 2, 1], [0, 0, -1]) == MISS                          # beside the triangle


def test_the_range_is_closed_at_both_ends():
    o, d = [0.25, 0.25, 1], [0, 0, -1]
    hit = (1.0, 0, [0.5, 0.25, 0.25])
    assert one(o, d, trange=(1.0, 5.0)) == hit and one(o, d, trange=(0.0, 1.0)) == hit and one(o, d, trange=(1.0, 1.0)) == hit
    assert one(o, d, trange=(np.nextafter(1.0, 2.0), 5.0)) == MISS
    assert one(o, d, trange=(0.0, np.nextafter(1.0, 0.0))) == MISS
    assert one(o, d, trange=(2.0, 1.0)) == MISS                        # an empty range
    assert one(o, d, trange=(np.nan, 5.0)) == MISS
    # an origin on the surface with tmin = 0: the self-hit at t = 0
    assert one([0.25, 0.25, 0], d) == (0.0, 0, [0.5, 0.25, 0.25])
    # two parallel triangles: a range that cuts off the nearer one finds the farther
    v = np.concatenate([TRI_V, TRI_V + F32([0, 0, -1])])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    assert one(o, d, v, f)[:2] == (1.0, 0) and one(o, d, v, f, trange=(1.5, INF))[:2] == (2.0, 1)


def test_directions_that_hit_nothing_and_faces_that_are_never_hit():
    o = [0.25, 0.25, 1]
    for d in ([0, 0, 0], [0, 0, -0.0], [np.nan, 0, -1], [0, np.inf, -1], [0, 0, -np.inf]):
        assert one(o, d) == MISS
    for f in ([[0, 1, 1]], [[2, 2, 2]], [[0, 0, 1]]):                   # a repeated index
        assert one(o, [0, 0, -1], f=np.array(f)) == MISS
    collinear = np.array([[0, 0, 0], [0.5, 0.5, 0], [1, 1, 0]], dtype=F32)
    assert one([0.5, 0.5, 1], [0, 0, -1], collinear) == MISS          # zero area, the ray through it
    # a non-finite origin hits nothing either
    assert one([np.nan, 0.25, 1], [0, 0, -1]) == MISS and one([np.inf, 0.25, 1], [0, 0, -1]) == MISS


def ico():
    v, f = synthetic.icosphere(8)
    return synthetic.perturb(v, radial=0.05, seed=2).astype(F32), np.asarray(f, dtype=np.int64)


def inside_rays(v, f):
    """from a point inside the mesh at every vertex and every edge midpoint, directions rounded to fp32"""
    o = np.array([0.0625, -0.03125, 0.09375], dtype=F32)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    v64 = v.astype(np.float64)
    targets = np.concatenate([v64, (v64[e[:, 0]] + v64[e[:, 1]]) * 0.5])
    D = (targets - o.astype(np.float64)).astype(F32)
    return np.broadcast_to(o, D.shape).copy(), D


def test_no_ray_from_inside_slips_between_two_faces():
    """642 rays at the vertices and 1920 at the edge midpoints of the perturbed icosphere, from inside: a closed mesh, so every ray must
    hit. The cap is zero misses -- the edge functions of two faces on a shared edge are exact negatives of each other"""
    v, f = ico()
    O, D = inside_rays(v, f)
    assert O.shape[0] == 642 + 1920
    t, I, W = rs.closest(O, D, v, f)
    misses = int((I < 0).sum())
    print(f"{O.shape[0]} rays, {misses} misses, t in [{t.min():.4f}, {t.max():.4f}]")
    assert misses == 0
    assert np.array_equal(rs.any_hit(O, D, v, f), I >= 0)
    assert (t > 0.5).all() and (t < 1.5).all() and (W >= 0).all() and np.abs(W.sum(1) - 1).max() <= 4 * 2.0 ** -52


def test_the_gradient_terms_are_the_derivatives_of_the_closed_form():
    """t = n . (a - o) / (n . d) with the face fixed, n = (b - a) x (c - a), differentiated by torch autograd in fp64, on rays with
    |n^ . d^| >= 0.1. Relative tolerance 1e-10: an expression of about 50 fp64 operations, amplified by at most 1 / 0.1^2, stays orders of
    magnitude below it. Per ray the scale is its largest term; per vertex the sum of the magnitudes of the terms it receives"""
    v, f = ico()
    rng = np.random.default_rng(3)
    n = 2000
    O = rng.uniform(-0.3, 0.3, (n, 3)).astype(F32)
    D = rng.normal(size=(n, 3)).astype(F32) * rng.uniform(0.5, 2.0, (n, 1)).astype(F32)
    t, I, W = rs.closest(O, D, v, f)
    assert (I >= 0).all()
    v64, d64 = v.astype(np.float64), D.astype(np.float64)
    nrm = np.cross(v64[f[I, 1]] - v64[f[I, 0]], v64[f[I, 2]] - v64[f[I, 0]])
    cosine = np.abs((nrm * d64).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d64, axis=1))
    keep = cosine >= 0.1
    assert keep.sum() > 0.9 * n
    O, D, t, I, W = O[keep], D[keep], t[keep], I[keep], W[keep]
    g = rng.uniform(-1.0, 2.0, O.shape[0])
    tO, tD, tV = rs.terms(O, D, v, f, I, W, t, g)
    tO_, tD_, tV_ = (torch.from_numpy(x) for x in (O.astype(np.float64), D.astype(np.float64), v64))
    for x in (tO_, tD_, tV_):
        x.requires_grad_()
    tf, tI = torch.from_numpy(f), torch.from_numpy(I)
    a, b, c = tV_[tf[tI, 0]], tV_[tf[tI, 1]], tV_[tf[tI, 2]]
    nn = torch.linalg.cross(b - a, c - a)
    closed = (nn * (a - tO_)).sum(1) / (nn * tD_).sum(1)
    assert np.abs(closed.detach().numpy() - t).max() <= 1e-12 * np.abs(t).max()
    (torch.from_numpy(g) * closed).sum().backward()
    for got, want in ((tO, tO_.grad.numpy()), (tD, tD_.grad.numpy())):
        rel = np.abs(got - want).max(1) / np.abs(want).max(1)
        print(f"largest relative deviation per ray {rel.max():.3e}")
        assert rel.max() <= 1e-10
    gV, sV = np.zeros_like(v64), np.zeros(v.shape[0])
    for k in range(3):
        np.add.at(gV, f[I, k], tV[:, k])
        np.add.at(sV, f[I, k], np.abs(tV[:, k]).max(1))
    dev = np.abs(gV - tV_.grad.numpy()).max(1)
    assert (dev[sV == 0] == 0).all()
    print(f"largest relative deviation per vertex {(dev[sV > 0] / sV[sV > 0]).max():.3e}")
    assert (dev[sV > 0] <= 1e-10 * sV[sV > 0]).all()
    # a miss has zero terms
    z = rs.terms(O[:2], D[:2], v, f, np.array([-1, f.shape[0]]), W[:2], np.array([INF, INF]), g[:2])
    assert not any(x.any() for x in z)


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_the_module_has_the_documented_symbols():
    from largesteps import raycast
    from largesteps.distance import MeshDistance
    assert issubclass(raycast.RayMesh, MeshDistance)
    assert list(inspect.signature(raycast.RayMesh.intersect).parameters) == ["self", "O", "D", "tmin", "tmax"]
    assert list(inspect.signature(raycast.RayMesh.occluded).parameters) == ["self", "O", "D", "tmin", "tmax"]
    sig = inspect.signature(raycast.ray_mesh_intersect)
    assert list(sig.parameters) == ["O", "D", "V", "F", "tmin", "tmax"] and sig.parameters["tmin"].default == 0.0 and sig.parameters["tmax"].default == math.inf
    sig = inspect.signature(raycast.ambient_occlusion)
    assert list(sig.parameters) == ["V", "F", "P", "N", "n_rays", "seed", "eps"] and sig.parameters["seed"].default == 0 and sig.parameters["eps"].default == 1e-4
    for name in ("update", "close", "squared_distance", "__enter__", "_check_source"):
        assert getattr(raycast.RayMesh, name) is getattr(MeshDistance, name)
    assert "O + t" in raycast.RayMesh.intersect.__doc__ and "t = 0" in raycast.RayMesh.intersect.__doc__


def test_argument_errors_are_raised_before_any_device_work():
    from largesteps.raycast import ambient_occlusion, ray_mesh_intersect
    v, f = TRI_V, TRI_F
    O, D = np.zeros((4, 3), F32), np.ones((4, 3), F32)
    with pytest.raises(ValueError):
        ray_mesh_intersect(np.zeros((4, 2)), D, v, f)
    with pytest.raises(ValueError):
        ray_mesh_intersect(O, np.ones((3, 3)), v, f)
    with pytest.raises(ValueError):
        ray_mesh_intersect(O, np.ones(3), v, f)
    with pytest.raises(TypeError):
        ray_mesh_intersect(O.astype(np.complex64), D, v, f)
    with pytest.raises(TypeError):
        ray_mesh_intersect(O, [["a", "b", "c"]] * 4, v, f)
    with pytest.raises(ValueError):
        ray_mesh_intersect(O, D, v, f, tmin=np.zeros(3))
    with pytest.raises(ValueError):
        ray_mesh_intersect(O, D, v, f, tmax=np.zeros((4, 1)))
    with pytest.raises(TypeError):
        ray_mesh_intersect(O, D, v, f, tmin="0")
    with pytest.raises(TypeError):
        ray_mesh_intersect(O, D, v, f, tmax=None)
    with pytest.raises(ValueError):
        ambient_occlusion(v, f, O, D, 0)
    with pytest.raises(TypeError):
        ambient_occlusion(v, f, O, D, 8.0)
    with pytest.raises(ValueError):
        ambient_occlusion(v, f, O, D[:3], 8)
    with pytest.raises(ValueError):
        ambient_occlusion(v, f, O, D, 8, eps=-1.0)
    with pytest.raises(TypeError):
        ambient_occlusion(v, f, O, D, 8, seed=0.5)
    with pytest.raises(ValueError):
        ambient_occlusion(v, np.zeros((1, 4), np.int64), O, D, 8)


def test_cpu_tensors_raise():
    from largesteps.raycast import RayMesh, ambient_occlusion, ray_mesh_intersect
    v, f = torch.from_numpy(TRI_V), torch.from_numpy(TRI_F)
    O, D = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ray_mesh_intersect(O, D, v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RayMesh(v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ambient_occlusion(v, f, O, D, 4)


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_mesh_ray_closest", "ls_mesh_ray_any", "ls_mesh_ray_backward_workspace_bytes", "ls_mesh_ray_backward"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(native.lib(), name).restype is ctypes.c_int
    assert native.lib().ls_version() == 110


def test_abi_argument_checks(native):
    lib = native.lib()
    E, OV = native.LS_E_INVALID, native.LS_E_OVERFLOW
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p(1)                  # never dereferenced: every call below fails an argument check first, or has nothing to do
    assert lib.ls_mesh_ray_closest(None, x, x, 1, None, x, x, x, None) == E
    assert lib.ls_mesh_ray_closest(h, None, x, 1, None, x, x, x, None) == E
    assert lib.ls_mesh_ray_closest(h, x, None, 1, None, x, x, x, None) == E
    assert lib.ls_mesh_ray_closest(h, x, x, -1, None, x, x, x, None) == E
    assert lib.ls_mesh_ray_closest(h, x, x, 2 ** 31, None, x, x, x, None) == OV
    assert lib.ls_mesh_ray_closest(h, None, None, 0, None, None, None, None, None) == 0
    assert lib.ls_mesh_ray_closest(h, x, x, 1, None, None, None, None, None) == 0           # every output NULL: nothing to do
    assert lib.ls_mesh_ray_any(None, x, x, 1, None, x, None) == E
    assert lib.ls_mesh_ray_any(h, None, x, 1, None, x, None) == E
    assert lib.ls_mesh_ray_any(h, x, None, 1, None, x, None) == E
    assert lib.ls_mesh_ray_any(h, x, x, 1, None, None, None) == E
    assert lib.ls_mesh_ray_any(h, x, x, -1, None, x, None) == E
    assert lib.ls_mesh_ray_any(h, x, x, 2 ** 31, None, x, None) == OV
    assert lib.ls_mesh_ray_any(h, None, None, 0, None, None, None) == 0
    n = ctypes.c_size_t(0)
    assert lib.ls_mesh_ray_backward_workspace_bytes(10, 4, None) == E
    assert lib.ls_mesh_ray_backward_workspace_bytes(-1, 4, ctypes.byref(n)) == E
    assert lib.ls_mesh_ray_backward_workspace_bytes(10, 0, ctypes.byref(n)) == E
    assert lib.ls_mesh_ray_backward_workspace_bytes(2 ** 31, 4, ctypes.byref(n)) == OV
    assert lib.ls_mesh_ray_backward_workspace_bytes(0, 4, ctypes.byref(n)) == 0 and n.value > 0
    small = n.value
    assert lib.ls_mesh_ray_backward_workspace_bytes(100000, 4000, ctypes.byref(n)) == 0
    assert n.value >= small + 100000 * (4 + 4) + 4000 * 36
    #                         handle O  D  n  I  W  t  g  vptr order gO gD gV ws bytes stream
    assert lib.ls_mesh_ray_backward(None, x, x, 1, x, x, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, None, x, 1, x, x, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, None, 1, x, x, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, None, x, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, x, None, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, x, x, None, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, -1, x, x, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    # the vertex gradient needs W, the corner ranking and a workspace
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, None, x, x, x, x, None, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, x, x, x, None, x, None, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, x, x, x, x, None, None, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_ray_backward(h, x, x, 1, x, x, x, x, x, x, None, None, x, None, 0, None) == E and "workspace" in native.last_error()
    assert lib.ls_mesh_ray_backward(h, x, x, 2 ** 31, x, x, x, x, x, x, x, x, x, x, 1 << 20, None) == OV
