"""
The point-to-mesh distance without a device: tests/distance_statement.py (the brute force the device must match bit for bit) against
closed forms -- a point above a plane, points inside and outside a cube, two parallel planes, a degenerate face, libigl's
vertex-to-surface Hausdorff distance on a V-shaped polygon and its hull -- its numpy and torch forms against each other, and the
boundary of largesteps.distance that answers before any device work: the C ABI's argument checks, the header and binding entries,
and the Python-side errors.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import distance_statement as ds
from largesteps import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def cube():
    """the cube [-1, 1]^3: 8 corners, 12 outward-oriented faces"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                  [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f


def flat(n=9):
    """an n x n grid on z = 0 over [0, 1]^2 (plane() without its sine)"""
    v, f = synthetic.plane(n)
    v[:, 2] = 0.0
    return v, f


def test_point_above_a_plane():
    v, f = flat()
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.uniform(0.05, 0.95, (200, 2)), rng.uniform(-2.0, 2.0, (200, 1))], 1).astype(F32)
    d2, I, C = ds.squared_distance(p, v, f)
    z = p[:, 2].astype(np.float64)
    assert np.array_equal(d2, z * z)
    assert np.array_equal(C[:, :2], p[:, :2].astype(np.float64)) and np.array_equal(C[:, 2], np.zeros(200))
    # the face found holds the foot of the point
    a, b, c = (v[f[I, k]].astype(np.float64) for k in range(3))
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    assert ((C >= lo) & (C <= hi)).all()


def test_points_inside_and_outside_a_cube():
    v, f = cube()
    rng = np.random.default_rng(1)
    inside = rng.uniform(-0.9, 0.9, (300, 3)).astype(F32)
    d2, _, _ = ds.squared_distance(inside, v, f)
    want = (1.0 - np.abs(inside.astype(np.float64))).min(1)
    assert np.allclose(np.sqrt(d2), want, rtol=1e-12, atol=1e-12)
    outside = rng.uniform(-4.0, 4.0, (600, 3)).astype(F32)
    outside = outside[(np.abs(outside) > 1.0).any(1)]
    d2, _, C = ds.squared_distance(outside, v, f)
    want = np.linalg.norm(np.maximum(np.abs(outside.astype(np.float64)) - 1.0, 0.0), axis=1)
    assert np.allclose(np.sqrt(d2), want, rtol=1e-12, atol=1e-12)
    assert np.allclose(C, np.clip(outside.astype(np.float64), -1.0, 1.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("d", [0.25, 1e-3, 3.0])
def test_parallel_planes_are_their_offset_apart(d):
    v, f = flat()
    w = v.copy()
    w[:, 2] = F32(d)
    assert ds.hausdorff(v, f, w, f) == float(F32(d))
    assert ds.hausdorff(w, f, v, f) == float(F32(d))


def test_a_segment_shaped_face_is_measured_as_its_segment():
    a, b = np.array([0.0, 0.0, 0.0]), np.array([2.0, 1.0, 0.5])
    faces = {"repeated": ([a, b], [[0, 0, 1]]), "repeated_last": ([a, b], [[0, 1, 1]]), "collinear": ([a, b, (a + b) / 2], [[0, 2, 1]]),
             "point": ([a], [[0, 0, 0]])}
    rng = np.random.default_rng(2)
    p = rng.normal(scale=2.0, size=(400, 3)).astype(F32)
    pp = p.astype(np.float64)
    for name, (v, f) in faces.items():
        v, f = np.asarray(v, dtype=F32), np.asarray(f)
        d2, I, C = ds.squared_distance(p, v, f)
        assert np.isfinite(d2).all() and np.isfinite(C).all() and (I == 0).all(), name
        if name == "point":
            want = ((pp - a) ** 2).sum(1)
        else:
            t = np.clip((pp - a) @ (b - a) / ((b - a) @ (b - a)), 0.0, 1.0)
            want = ((pp - (a + t[:, None] * (b - a))) ** 2).sum(1)
        assert np.allclose(d2, want, rtol=1e-12, atol=1e-15), name
    # the region tests alone would give NaN on the repeated index; the statement's rule keeps them off that face
    v, f = np.asarray([a, b], dtype=np.float64), np.asarray([[0, 0, 1]])
    with np.errstate(all="ignore"):
        raw = ds.rs.point_triangle(pp[:, None], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])
    assert np.isnan(raw).any()


def test_a_degenerate_face_next_to_a_proper_one_keeps_the_tie_rule():
    """a degenerate face that shares an edge with a proper one: points whose nearest point is on the shared edge tie at the lower id"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]], dtype=F32)
    for f, lowest in (([[0, 1, 2], [0, 1, 3]], 0), ([[0, 1, 3], [0, 1, 2]], 0)):
        p = np.array([[0.5, -1.0, 0.0], [0.25, -0.5, 0.5]], dtype=F32)
        d2, I, C = ds.squared_distance(p, v, np.asarray(f))
        assert (I == lowest).all()
        assert np.array_equal(C[:, 1], [0.0, 0.0])


def test_the_vertex_based_value_of_a_v_polygon_against_its_hull():
    """libigl's hausdorff queries vertices only: a V-shaped polygon and its convex hull share every hull corner and the notch lies
    inside the hull, so the value is 0, though the hull's edge across the notch is 1/sqrt(2) from the polygon"""
    V = np.array([[-1, 1, 0], [0, -1, 0], [1, 1, 0], [0, 0, 0]], dtype=F32)
    FV = np.array([[0, 1, 3], [1, 2, 3]])
    H = V[:3]
    FH = np.array([[0, 1, 2]])
    assert ds.hausdorff(V, FV, H, FH) == 0.0
    assert ds.hausdorff(H, FH, V, FV) == 0.0
    d2, _, _ = ds.squared_distance(np.array([[0, 1, 0]], dtype=F32), V, FV)
    assert math.isclose(math.sqrt(d2[0]), 1 / math.sqrt(2), rel_tol=1e-12)


def test_numpy_and_torch_statements_agree_bitwise():
    v, f = synthetic.icosphere(4)
    v = synthetic.perturb(v, radial=0.05, seed=5).astype(F32)
    f = np.concatenate([f, [[0, 0, 1], [3, 3, 3]]])             # two degenerate faces
    rng = np.random.default_rng(3)
    p = np.concatenate([v[:50], (v[f[:40, 0]] + v[f[:40, 1]]) / 2, rng.normal(scale=1.5, size=(100, 3))]).astype(F32)
    want = ds.squared_distance(p, v, f, chunk=37)
    got = ds.squared_distance_torch(p, v, f, "cpu", pchunk=53, tchunk=61)
    for w, g in zip(want, got):
        assert np.array_equal(w, g.numpy())
    assert np.isfinite(want[0]).all()
    w, g = synthetic.icosphere(3)
    w = (w * F32(1.1)).astype(F32)
    assert ds.hausdorff(v, f, w, g) == ds.hausdorff(v, f, w, g, squared=ds.squared_on("cpu", pchunk=64, tchunk=64))


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_mesh_distance_create", "ls_mesh_distance_query", "ls_mesh_distance_max", "ls_mesh_distance_destroy"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(native.lib(), name).restype is ctypes.c_int


def test_abi_argument_checks(native):
    lib = native.lib()
    h = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 9)()
    idx = (ctypes.c_int32 * 3)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(idx, ctypes.c_void_p)
    E = native.LS_E_INVALID
    assert lib.ls_mesh_distance_create(None, 3, q, 4, 1, 0, None, ctypes.byref(h)) == E
    assert lib.ls_mesh_distance_create(p, 3, None, 4, 1, 0, None, ctypes.byref(h)) == E
    assert lib.ls_mesh_distance_create(p, 3, q, 4, 1, 0, None, None) == E
    assert lib.ls_mesh_distance_create(p, 3, q, 2, 1, 0, None, ctypes.byref(h)) == E
    assert lib.ls_mesh_distance_create(p, 3, q, 4, 0, 0, None, ctypes.byref(h)) == E and "no faces" in native.last_error()
    assert lib.ls_mesh_distance_create(p, 0, q, 4, 1, 0, None, ctypes.byref(h)) == E
    assert h.value is None
    assert lib.ls_mesh_distance_create(p, 2 ** 31, q, 4, 1, 0, None, ctypes.byref(h)) == native.LS_E_OVERFLOW
    d = (ctypes.c_double * 1)()
    assert lib.ls_mesh_distance_query(None, p, 1, d, None, None, None) == E
    assert lib.ls_mesh_distance_query(ctypes.c_void_p(1), None, 1, d, None, None, None) == E
    assert lib.ls_mesh_distance_query(ctypes.c_void_p(1), p, -1, d, None, None, None) == E
    assert lib.ls_mesh_distance_max(None, p, 1, d, None) == E
    assert lib.ls_mesh_distance_max(ctypes.c_void_p(1), p, 1, None, None) == E
    assert lib.ls_mesh_distance_destroy(None) == 0


def test_python_errors_before_the_device():
    from largesteps.distance import MeshDistance, hausdorff, point_mesh_squared_distance
    v, f = cube()
    with pytest.raises(ValueError, match="no faces"):
        point_mesh_squared_distance(v, v, np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match="no vertices"):
        hausdorff(np.zeros((0, 3)), f, v, f)
    with pytest.raises(ValueError, match="no vertices"):
        hausdorff(v, f, np.zeros((0, 3)), f)
    with pytest.raises(ValueError):
        MeshDistance(v[:, :2], f)
    with pytest.raises(TypeError):
        MeshDistance(v, f.astype(np.float32))
    with pytest.raises(RuntimeError, match="HIP device"):
        MeshDistance(torch.from_numpy(v), torch.from_numpy(f))
