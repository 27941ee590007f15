"""
The winding number of largesteps.distance without a device: the rule of tests/winding_statement.py against itself on shapes whose answer
is known (a cube from its centre, flipped, doubled, overlapping, open), the num == 0 cases, the walk against the exact sum, the error of
the far field as beta grows, and the public surface with the argument errors that are raised before any device work.
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import winding_statement as ws
from largesteps import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=F32)          # vertex 4 x + 2 y + z
# two faces per side, outward: -x, +x, -y, +y, -z, +z
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def tol(T, s):
    """the tolerance of a winding number of T terms against the statement: T 2^-50 max(1, sum |terms|) -- T additions that round once each
    and an atan2 a few ulp off on either side, with a factor 8 over that"""
    return T * 2.0 ** -50 * np.maximum(1.0, s)


def sphere(n=6, radial=0.05, seed=2):
    v, f = synthetic.icosphere(n)
    return synthetic.perturb(v, radial=radial, seed=seed).astype(F32), np.asarray(f, dtype=np.int64)


def mean_edge(v, f):
    v = v.astype(np.float64)
    return float(np.mean([np.linalg.norm(v[f[:, k]] - v[f[:, (k + 1) % 3]], axis=1).mean() for k in range(3)]))


def queries(v, f, seed=0, per=50, box=100):
    """fp32 (P, side): `per` face centroids moved 1/4, 1 and 4 mean edges along the face normal, outwards (side 0) and inwards (side 1),
    then `box` points in the mesh's box grown by half (side -1: unknown)"""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    h = mean_edge(v, f)
    P, side = [], []
    for k, dist in enumerate((0.25, 1.0, 4.0)):
        ids = rng.choice(f.shape[0], per)
        a, b, c = v64[f[ids, 0]], v64[f[ids, 1]], v64[f[ids, 2]]
        nrm = np.cross(b - a, c - a)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        for s, sign in ((0, 1.0), (1, -1.0)):
            P.append((a + b + c) / 3 + sign * dist * h * nrm)
            side.append(np.full(per, s))
    lo, hi = v64.min(0), v64.max(0)
    P.append((lo + hi) / 2 + rng.uniform(-0.75, 0.75, (box, 3)) * (hi - lo))
    side.append(np.full(box, -1))
    return np.concatenate(P).astype(F32), np.concatenate(side)


def test_a_cube_from_its_centre_is_six_sixths():
    t = ws.solid_angles(np.array([[0.5, 0.5, 0.5]], dtype=F32), CUBE_V, CUBE_F)[0]
    sides = t.reshape(6, 2).sum(1)
    assert np.abs(sides - 1 / 6).max() <= 2.0 ** -50
    w, s = ws.exact(np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [2, 0.5, 0.5], [-3, 4, 5]], dtype=F32), CUBE_V, CUBE_F)
    assert np.abs(w - [1, 1, 0, 0]).max() <= 12 * 2.0 ** -50 and (s <= 1 + 2.0 ** -40).all()


def test_orientation_multiplicity_overlap_and_an_open_mesh():
    q = np.array([[0.5, 0.5, 0.5]], dtype=F32)
    assert abs(ws.exact(q, CUBE_V, CUBE_F[:, ::-1])[0][0] + 1) <= 12 * 2.0 ** -50                       # flipped
    assert abs(ws.exact(q, CUBE_V, np.concatenate([CUBE_F, CUBE_F]))[0][0] - 2) <= 24 * 2.0 ** -50      # listed twice
    v, f = sphere()
    v2 = np.concatenate([v, v + F32([1.0, 0, 0])])
    f2 = np.concatenate([f, f + v.shape[0]])
    P = np.array([[0.5, 0, 0], [-0.5, 0, 0], [1.5, 0, 0], [0.5, 2, 0]], dtype=F32)                     # overlap, first only, second only, neither
    w, _ = ws.exact(P, v2, f2)
    assert np.abs(w - [2, 1, 1, 0]).max() <= 1e-12
    cen = v.astype(np.float64)[f].mean(1)
    cap = f[cen[:, 2] > 0]                                                                           # the upper hemisphere, open
    w, _ = ws.exact(np.array([[0, 0, 0.01], [0, 0, 0.5], [0, 0, -0.5], [0, 0, 5]], dtype=F32), v, cap)
    assert 0.4 < w[0] < 0.6 and w[0] < w[1] < 1 and 0 < w[2] < w[0] and abs(w[3]) < 0.02


def test_the_exact_sum_is_an_integer_away_from_the_surface():
    """icosphere(6) with 5 % radial noise, 720 faces, queries at 1/4, 1 and 4 mean edges from the surface on both sides: within 1e-12 of
    1 inside and of 0 outside. The sum of 720 terms of size <= 1/2 rounds to about 720 2^-53 = 8e-14"""
    v, f = sphere()
    assert f.shape[0] == 720
    P, side = queries(v, f, seed=1)
    w, _ = ws.exact(P, v, f)
    known = side >= 0
    dev = np.abs(w[known] - side[known])
    print(f"exact: w - expected in [{(w[known] - side[known]).min():.2e}, {(w[known] - side[known]).max():.2e}]")
    assert dev.max() <= 1e-12
    assert np.abs(w[~known] - np.round(w[~known])).max() <= 1e-9              # box points may lie anywhere near the surface


def test_a_zero_numerator_contributes_zero_and_a_non_finite_query_is_nan():
    tri_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=F32)
    tri = np.array([[0, 1, 2]])
    P = np.array([[0.25, 0.25, 0], [5, 5, 0], [0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0]], dtype=F32)       # in the face, in its plane, vertex, edges
    assert (ws.solid_angles(P, tri_v, tri) == 0).all()
    above = ws.solid_angles(np.array([[0.25, 0.25, 2.0 ** -20], [0.25, 0.25, -2.0 ** -20]], dtype=F32), tri_v, tri)[:, 0]
    assert abs(above[0] + 0.5) < 1e-5 and abs(above[1] - 0.5) < 1e-5            # whose mean the in-plane value is (the normal side sees -1/2)
    for bad in ([[0, 1, 1]], [[2, 2, 2]], [[0, 3, 3]]):                         # repeated indices
        assert (ws.solid_angles(np.array([[0.3, 0.2, 0.7]], dtype=F32), tri_v, np.array(bad)) == 0).all()
    collinear = np.array([[0, 0, 0], [0.5, 0.5, 0], [1, 1, 0]], dtype=F32)
    assert (ws.solid_angles(np.array([[0.3, 0.2, 0.7]], dtype=F32), collinear, tri) == 0).all()
    q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5]], dtype=F32)
    w, _ = ws.exact(q, CUBE_V, CUBE_F)
    assert np.isnan(w[:3]).all() and abs(w[3] - 1) < 1e-12
    tree = ws.build_tree(CUBE_V, CUBE_F)
    w, _, acc, leaves = ws.walk(q, tree, ws.moments(tree), 2.0)
    assert np.isnan(w[:3]).all() and (acc[:3] == 0).all() and (leaves[:3] == 0).all() and abs(w[3] - 1) < 1e-12


def test_the_tree_builder_and_the_moments_of_simple_nodes():
    v, f = sphere()
    tree = ws.build_tree(v, f)
    T = f.shape[0]
    assert sorted(tree["tri"].tolist()) == list(range(T)) and tree["esc"][0] == -1
    lo, hi = ws.ranges(tree, T)
    assert lo[0] == 0 and hi[0] == T - 1
    m = ws.moments(tree)
    v64 = v.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]), axis=1)
    assert abs(m[0, ws.AR_] - area.sum()) <= 1e-12 * area.sum()
    assert np.abs(m[0, ws.N_:ws.N_ + 3]).max() <= 1e-12 * area.sum()                                # a closed mesh: the area vectors cancel
    # a leaf: p is the centroid, so C vanishes, N is the area vector, and r reaches every corner
    k = T - 1 + 5
    tri = v64[f[tree["tri"][5]]]
    assert np.abs(m[k, :3] - tri.mean(0)).max() <= 1e-14 and np.abs(m[k, ws.C_:ws.C_ + 9]).max() <= 1e-16
    assert (np.linalg.norm(tri - m[k, :3], axis=1) <= m[k, ws.R_]).all()
    # every node: r reaches the corners of all its faces
    for node in (0, 1, 7, T - 2):
        corners = v64[f[tree["tri"][lo[node]:hi[node] + 1]]].reshape(-1, 3)
        assert (np.linalg.norm(corners - m[node, :3], axis=1) <= m[node, ws.R_] * (1 + 1e-12)).all()
    # the trace of T_i.. against its definition for the root: sum a_i |x - p|^2 integrated
    one = ws.build_tree(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F32), np.array([[0, 1, 2]]))
    m1 = ws.moments(one)[0]
    # the unit right triangle about its centroid: integral of x^2 = 1/36, of x y = -1/72, area 1/2, normal +z
    assert np.allclose(m1[ws.T_ + 12:ws.T_ + 18], [1 / 36, -1 / 72, 0, 1 / 36, 0, 0], rtol=0, atol=1e-15) and not m1[ws.T_:ws.T_ + 12].any()


def test_the_walk_that_never_accepts_is_the_exact_sum():
    v, f = sphere()
    P, _ = queries(v, f, seed=2)
    tree = ws.build_tree(v, f)
    m = ws.moments(tree)
    we, se = ws.exact(P, v, f)
    ww, sw, acc, leaves = ws.walk(P, tree, m, 1e30)
    assert (acc == 0).all() and (leaves == f.shape[0]).all()
    assert (np.abs(ww - we) <= tol(f.shape[0], se)).all() and np.abs(sw - se).max() <= 1e-12


def test_the_far_field_error_shrinks_with_beta_and_keeps_the_sign():
    """the sign of signed_distance is right iff the error is below 0.5; 0.25 is half of that: a condition, not an accuracy claim"""
    v, f = sphere()
    P, _ = queries(v, f, seed=3)
    tree = ws.build_tree(v, f)
    m = ws.moments(tree)
    we, _ = ws.exact(P, v, f)
    errs = []
    for beta in (2.0, 3.0, 4.0):
        w, _, acc, leaves = ws.walk(P, tree, m, beta)
        e = np.abs(w - we)
        errs.append(e.max())
        print(f"beta {beta}: max error {e.max():.2e}, mean {e.mean():.2e}; {acc.mean():.0f} nodes accepted and {leaves.mean():.0f} leaves per query")
    assert errs[0] < 0.25 and errs[0] > errs[1] > errs[2]
    w1 = ws.walk(P, tree, m, 1.0)[0]                      # beta = 1: a node is accepted as soon as the query leaves its ball
    assert np.isfinite(w1).all()


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_the_module_has_the_documented_symbols():
    from largesteps import distance, raycast
    sig = inspect.signature(distance.MeshDistance.winding_number)
    assert list(sig.parameters) == ["self", "P", "beta"] and sig.parameters["beta"].default == 2.0
    sig = inspect.signature(distance.MeshDistance.signed_distance)
    assert list(sig.parameters) == ["self", "P", "beta"] and sig.parameters["beta"].default == 2.0
    sig = inspect.signature(distance.winding_number)
    assert list(sig.parameters) == ["V", "F", "P", "beta"] and sig.parameters["beta"].default == 2.0
    sig = inspect.signature(distance.signed_distance)
    assert list(sig.parameters) == ["P", "V", "F", "beta"] and sig.parameters["beta"].default == 2.0
    for name in ("winding_number", "signed_distance"):
        assert getattr(raycast.RayMesh, name) is getattr(distance.MeshDistance, name)
    assert "1 - 2 w" in distance.MeshDistance.signed_distance.__doc__


def test_argument_errors_are_raised_before_any_device_work():
    from largesteps.distance import signed_distance, winding_number
    v, f, P = CUBE_V, CUBE_F, np.zeros((4, 3), F32)
    for beta in (0.5, 0.0, -2.0, math.nan, -math.inf):
        with pytest.raises(ValueError, match="beta"):
            winding_number(v, f, P, beta)
        with pytest.raises(ValueError, match="beta"):
            signed_distance(P, v, f, beta)
    for beta in ("2", None, [2.0], True):
        with pytest.raises(TypeError):
            winding_number(v, f, P, beta)
    with pytest.raises(ValueError):
        winding_number(v, f, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        signed_distance(np.zeros(3), v, f)
    with pytest.raises(TypeError):
        winding_number(v, f, P.astype(np.complex64))
    with pytest.raises(ValueError):
        winding_number(v, np.zeros((2, 4), np.int64), P)
    with pytest.raises(TypeError):
        signed_distance(P, v, f.astype(np.float64))


def test_cpu_tensors_raise():
    from largesteps.distance import signed_distance, winding_number
    v, f, P = torch.from_numpy(CUBE_V), torch.from_numpy(CUBE_F), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        winding_number(v, f, P)
    with pytest.raises(RuntimeError, match="no CPU path"):
        signed_distance(P, v, f)


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_mesh_winding_bytes", "ls_mesh_winding_prepare", "ls_mesh_winding_query", "ls_mesh_winding_exact", "ls_mesh_winding_arrays"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert getattr(native.lib(), name).restype is ctypes.c_int
    assert sorted(n for n in native.EXPORTED_SYMBOLS if n.startswith("ls_mesh_winding_")) == sorted(NAMES)


def test_abi_argument_checks(native):
    lib = native.lib()
    E, OV = native.LS_E_INVALID, native.LS_E_OVERFLOW
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p(1)                  # never dereferenced: every call below fails an argument check first, or has nothing to do
    n = ctypes.c_size_t(0)
    assert lib.ls_mesh_winding_bytes(4, None) == E
    assert lib.ls_mesh_winding_bytes(0, ctypes.byref(n)) == E
    assert lib.ls_mesh_winding_bytes(2 ** 31, ctypes.byref(n)) == OV
    assert lib.ls_mesh_winding_bytes(1, ctypes.byref(n)) == 0 and n.value >= 36 * 8 + 4
    assert lib.ls_mesh_winding_bytes(1000, ctypes.byref(n)) == 0 and n.value >= 1999 * 36 * 8 + 4000
    assert lib.ls_mesh_winding_prepare(None, x, None) == E
    assert lib.ls_mesh_winding_prepare(h, None, None) == E
    for beta in (0.5, -1.0, math.nan):
        assert lib.ls_mesh_winding_query(h, x, x, 1, beta, x, None) == E and "beta" in native.last_error()
    assert lib.ls_mesh_winding_query(None, x, x, 1, 2.0, x, None) == E
    assert lib.ls_mesh_winding_query(h, None, x, 1, 2.0, x, None) == E
    assert lib.ls_mesh_winding_query(h, x, None, 1, 2.0, x, None) == E
    assert lib.ls_mesh_winding_query(h, x, x, 1, 2.0, None, None) == E
    assert lib.ls_mesh_winding_query(h, x, x, -1, 2.0, x, None) == E
    assert lib.ls_mesh_winding_query(h, x, x, 2 ** 31, 2.0, x, None) == OV
    assert lib.ls_mesh_winding_query(h, x, None, 0, 2.0, None, None) == 0
    assert lib.ls_mesh_winding_query(h, None, None, 0, math.inf, None, None) == 0            # the exact kernel needs no moments
    assert lib.ls_mesh_winding_exact(None, x, 1, x, None) == E
    assert lib.ls_mesh_winding_exact(h, None, 1, x, None) == E
    assert lib.ls_mesh_winding_exact(h, x, 1, None, None) == E
    assert lib.ls_mesh_winding_exact(h, x, -1, x, None) == E
    assert lib.ls_mesh_winding_exact(h, x, 2 ** 31, x, None) == OV
    assert lib.ls_mesh_winding_exact(h, None, 0, None, None) == 0
    assert lib.ls_mesh_winding_arrays(None, x, x, x, x, x, x, x, None) == E
    assert lib.ls_mesh_winding_arrays(h, None, None, None, None, None, None, x, None) == E      # the moments without their buffer
