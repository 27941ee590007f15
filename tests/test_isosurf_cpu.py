"""
The isosurface extractor of largesteps.levelset without a device: the rule of tests/isosurf_statement.py on fields whose level set is
known (closed, oriented, of the right genus, as accurate as linear interpolation allows), at the grid's boundary, at non-finite nodes
and at S == iso; its analytic gradient against central differences; the condition on the input of the repair test of
tests/test_isosurf_gpu.py; and the public surface with the argument errors that come before any device work.
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import isosurf_statement as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def torus_sdf(shape, centre, R, r):
    p = st.grid_points(shape) - np.asarray(centre, dtype=np.float64)
    return (np.hypot(np.hypot(p[..., 0], p[..., 1]) - R, p[..., 2]) - r).astype(F32)


def two_spheres_sdf(shape):
    a = st.sphere_sdf(shape, (4.3, 5.1, 5.6), 2.7)
    b = st.sphere_sdf(shape, (7.2, 6.4, 5.9), 2.4)
    return np.minimum(a, b)


CLOSED = {   # name -> (field, Euler characteristic)
    "sphere9": (lambda: st.sphere_sdf((9, 9, 9), (4.2, 3.9, 4.1), 0.33 * 9), 2),
    "sphere12": (lambda: st.sphere_sdf((12, 12, 12), (5.3, 5.8, 5.6), 0.33 * 12), 2),
    "torus": (lambda: torus_sdf((16, 16, 9), (7.4, 7.7, 4.2), 4.6, 1.9), 0),
    "union": (lambda: two_spheres_sdf((12, 12, 12)), 2),
}


def check_closed_and_oriented(S, V, F, T, chi):
    """every directed edge once and its reverse once, the Euler characteristic, a positive volume, every normal from low to high"""
    assert F.shape[0] > 0 and st.boundary_edges(F).shape[0] == 0
    assert st.euler(V, F) == chi
    assert st.signed_volume(V, F) > 0
    assert np.unique(F).size == V.shape[0]                                   # no vertex without a face
    nodes = st.tet_nodes(S.shape, T)
    pos = st.grid_points(S.shape).reshape(-1, 3)[nodes]                      # (m, 4, 3)
    low = (S.reshape(-1)[nodes] < 0)[..., None]
    to_high = (pos * ~low).sum(1) / (~low).sum(1) - (pos * low).sum(1) / low.sum(1)
    v = V.astype(np.float64)
    normal = np.cross(v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]])
    assert (np.einsum("ij,ij->i", normal, to_high) > 0).all()


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_and_oriented(name):
    make, chi = CLOSED[name]
    S = make()
    V, E, F, T = st.extract(S, with_tets=True)
    print(f"{name}: {V.shape[0]} vertices, {F.shape[0]} faces")
    check_closed_and_oriented(S, V, F, T, chi)
    assert (np.diff(E) > 0).all() and (np.diff(T) >= 0).all()               # the orders of rule 4 and rule 5


def test_the_tables_of_the_device_source_are_the_statements():
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "isosurf.hip")).read()

    def numbers(name):
        body = re.search(name + r"(?:\[\d+\])?\s*=\s*\{?([^;]*?)\}?;", src).group(1)
        return [int(x) for x in re.findall(r"\d+", body)]
    case, edge, corner, neg = st.packed_tables()
    assert numbers("ISO_CASE") == case and numbers("ISO_EDGE") == edge and numbers("ISO_CORNER") == corner
    assert numbers("ISO_NEG") == [neg]
    assert numbers("ISO_SLOT_CORNER") == [int(4 * d[0] + 2 * d[1] + d[2]) for d in st.SLOTS]


@pytest.mark.parametrize("n", [9, 12])
def test_sphere_vertices_lie_within_the_interpolation_bound(n):
    """Along an edge of length l <= sqrt(3) h the distance to the centre, f, has a second derivative of at most 1 / rho, rho the
    distance of the edge from the centre, which is at least r - sqrt(3) h for an edge that crosses the sphere. The linear interpolant
    of f between the ends is therefore off by at most l^2 / (8 rho) <= 3 h^2 / (8 (r - sqrt(3) h)), and f being a distance, the point
    where the interpolant vanishes is that far from the sphere at most. Here h = 1. The fp32 rounding of S and of the positions
    (1e-6) is far below the bound's slack."""
    c, r = np.array([4.2, 3.9, 4.1]) * n / 9, 0.33 * n
    V, _, _ = st.extract(st.sphere_sdf((n, n, n), c, r))
    err = np.abs(np.linalg.norm(V.astype(np.float64) - c, axis=1) - r).max()
    bound = 3.0 / (8.0 * (r - math.sqrt(3.0)))
    print(f"n = {n}: largest distance from the sphere {err:.4f}, bound {bound:.4f}")
    assert err <= bound


def test_a_surface_that_leaves_the_grid_has_its_boundary_on_the_grids():
    shape = (8, 7, 9)
    S = st.sphere_sdf(shape, (1.3, 3.1, 7.6), 3.4)
    V, E, F = st.extract(S)
    be = st.boundary_edges(F)
    assert be.shape[0] > 0
    top = np.array(shape, dtype=F32) - 1
    on = np.concatenate([V == 0, V == top], 1)                                # (n, 6): on which faces of the grid a vertex lies
    assert (on[be[:, 0]] & on[be[:, 1]]).any(1).all()                        # both ends of a boundary edge on one face of the grid


def test_non_finite_nodes_remove_exactly_the_cubes_around_them():
    shape = (9, 9, 9)
    clean = st.sphere_sdf(shape, (4.2, 3.9, 4.1), 2.97)
    S = clean.copy()
    bad = [(4, 4, 1), (1, 4, 4), (6, 5, 6), (4, 7, 4)]
    for (i, j, k), x in zip(bad, (np.nan, np.inf, -np.inf, np.nan)):
        S[i, j, k] = x
    Vc, Ec, Fc, Tc = st.extract(clean, with_tets=True)
    V, E, F, T = st.extract(S, with_tets=True)
    ci, cj, ck = np.unravel_index(Tc // 6, (8, 8, 8))
    hit = np.zeros(Tc.shape[0], bool)
    for i, j, k in bad:
        hit |= (np.abs(ci + 0.5 - i) < 1) & (np.abs(cj + 0.5 - j) < 1) & (np.abs(ck + 0.5 - k) < 1)
    assert hit.any() and np.array_equal(T, Tc[~hit])
    assert np.array_equal(E[F], Ec[Fc[~hit]])                                 # the same grid edges, hence the same positions
    assert np.array_equal(V[F], Vc[Fc[~hit]])
    assert np.isfinite(V).all() and np.isin(E, Ec).all()


def test_iso_exactly_at_a_node_follows_the_low_high_rule():
    rng = np.random.default_rng(3)
    S = rng.integers(-2, 3, (6, 7, 5)).astype(F32)
    iso = 1.0
    V, E, F, T = st.extract(S, iso, with_tets=True)
    mask, _ = st.classify(S, iso)
    at = (S == iso).reshape(-1)
    assert at.sum() > 20
    a, s = E // 8, E % 8
    b = a + (st.SLOTS[s] * [35, 5, 1]).sum(1)
    Sf = S.reshape(-1)
    assert ((Sf[a] < iso) != (Sf[b] < iso)).all()                             # S == iso counts as high
    nodes = st.grid_points(S.shape).reshape(-1, 3).astype(F32)
    assert np.array_equal(V[at[a]], nodes[a[at[a]]]) and np.array_equal(V[at[b]], nodes[b[at[b]]])      # t = 0 or t = 1: on the node
    v = V.astype(np.float64)
    area = np.linalg.norm(np.cross(v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]]), axis=1)
    assert (area == 0).any() and (area > 0).any()
    # the connectivity is that of an iso just below the value: S == iso is the limit from the side on which the node is high
    V2, E2, F2 = st.extract(S, iso - 0.25)
    assert np.array_equal(E2, E) and np.array_equal(F2, F)


def gradient_case():
    """a field whose low values lie in [-1, -0.5] and whose high values in [0.5, 1]: every live edge has |S[b] - S[a]| >= 1 and
    0.25 <= t <= 0.75, so no t is near 0 or 1 and the fp64 form is smooth over the steps of the differences"""
    rng = np.random.default_rng(11)
    shape = (6, 7, 5)
    sign = np.where(st.sphere_sdf(shape, (2.4, 3.1, 2.2), 2.1) < 0, -1.0, 1.0)
    S = (sign * (0.5 + 0.5 * rng.random(shape))).astype(F32)
    return S, (0.3, -1.0, 2.0), (0.7, 1.3, 0.9)


def test_gradient_against_central_differences():
    """The statement's analytic gradient (fp64) against central differences of its fp64 form. L = sum <gV, V> is a sum of terms
    c (iso - S[a]) / (S[b] - S[a]) with |S[b] - S[a]| >= 1 and |c| of order 1, up to 14 of them per node. With the step 1e-5 the
    truncation error of a central difference is step^2 / 6 x (third derivative) <= 1e-10 / 6 x 6 |c| x 14, about 1e-9, and its rounding
    error is eps |L| / step, 2e-16 x 1e2 / 1e-5 = 2e-9 for the |L| of a few hundred terms. Observed on the CPU this was written on:
    1.5e-9 against a largest component of 2.7. The tolerance is 2e-8 absolute: 13 x what was observed, which leaves room for another
    libm and another order of the sums in L, and still sits eight orders below the size of the gradient -- a wrong sign, a swapped
    end or a missing term is off by order 1."""
    S, origin, spacing = gradient_case()
    V, E, F = st.extract(S, 0.0, origin, spacing)
    t = (V.astype(np.float64) - st.vertices64(S, 0.0, origin, spacing, E))
    assert np.abs(t).max() < 1e-5                                             # the fp32 positions are the fp64 form's, rounded
    rng = np.random.default_rng(12)
    gV = rng.standard_normal(V.shape)
    S64 = S.astype(np.float64)
    g = st.grad64(S64, 0.0, spacing, E, gV)
    step = 1e-5
    num = np.zeros_like(S64)
    for idx in np.ndindex(S64.shape):
        up, dn = S64.copy(), S64.copy()
        up[idx] += step
        dn[idx] -= step
        num[idx] = ((gV * st.vertices64(up, 0.0, origin, spacing, E)).sum() - (gV * st.vertices64(dn, 0.0, origin, spacing, E)).sum()) / (2 * step)
    err = np.abs(num - g).max()
    print(f"analytic against central differences: {err:.3e}, largest component {np.abs(g).max():.3e}")
    assert np.abs(g).max() > 1 and err <= 2e-8
    # the device's rule (fp64 terms from the fp32 inputs, a fixed order, one rounding to fp32) is that gradient rounded
    g32 = st.grad_S(S, 0.0, spacing, gV.astype(F32))
    g_of_f32 = st.grad64(S64, 0.0, spacing, E, gV.astype(F32).astype(np.float64))
    assert np.abs(g32 - g_of_f32).max() <= 2.0 ** -23 * np.abs(g_of_f32).max()
    assert (g32.reshape(-1)[np.setdiff1d(np.arange(S.size), np.concatenate([E // 8, E // 8 + (st.SLOTS[E % 8] * [35, 5, 1]).sum(1)]))] == 0).all()


def test_the_repair_case_meets_its_condition():
    """tests/test_isosurf_gpu.py repairs selfx_statement.two_spheres() with h = 3 / 16 and beta = inf. The condition on that input, checked
    here on the statement's own pipeline (the numpy winding number, this extractor, the numpy self-intersection rule): no grid node
    lies on the mesh (every winding number is an integer to 1e-12, so the device's field has the same fp32 values), no t is exactly 0
    or 1, and the result has no reported pair. h = 3 / 16 makes every coordinate of the result exact in fp32, so that coplanar faces
    of the staircase have det == 0 exactly and are not reported."""
    import selfx_statement as sx
    import winding_statement as wn
    v, f = sx.two_spheres()
    h = 0.1875
    origin, dims, P = st.level_set_grid(v, h)
    w, _ = wn.exact(P, v, f)
    assert np.abs(w - np.round(w)).max() < 1e-12
    S = (0.5 - w).astype(F32).reshape(dims)
    assert set(np.unique(S)) == {-1.5, -0.5, 0.5}
    V, E, F, T = st.extract(S, 0.0, origin, h, with_tets=True)
    t = st.vertices64(S, 0.0, (0, 0, 0), 1.0, E) - np.stack(np.unravel_index(E // 8, dims), 1)
    t = t.max(1)
    assert ((t > 0) & (t < 1)).all()
    assert np.array_equal(V.astype(np.float64), st.vertices64(S, 0.0, origin, h, E))      # exact coordinates
    assert (V.shape[0], F.shape[0]) == (1814, 3624)
    assert st.boundary_edges(F).shape[0] == 0 and st.euler(V, F) == 2 and st.signed_volume(V, F) > 0
    assert sx.pairs_fast(V, F).shape == (0, 2)


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_the_module_has_the_documented_symbols():
    from largesteps import levelset
    sig = inspect.signature(levelset.isosurface)
    assert list(sig.parameters) == ["S", "iso", "origin", "spacing", "return_edges"]
    assert [p.default for p in sig.parameters.values()][1:] == [0.0, (0.0, 0.0, 0.0), 1.0, False]
    sig = inspect.signature(levelset.remesh_level_set)
    assert list(sig.parameters) == ["V", "F", "h", "field", "offset", "pad", "beta"]
    assert [p.default for p in sig.parameters.values()][3:] == ["winding", 0.0, 2, 2.0]
    for words in ("zero area", "not capturable", "synchronises once", "Bitwise reproducible"):
        assert words in levelset.isosurface.__doc__, words
    for words in ("closed", "distinct\n    tets", "as fine as h", "poorly shaped", "remesh_botsch", "smallest h that fits"):
        assert words in levelset.remesh_level_set.__doc__, words
    for words in ("Kuhn split", "no float atomics", "not capturable", "CPU tensors raise"):
        assert words in levelset.__doc__, words


def test_argument_errors_are_raised_before_any_device_work():
    from largesteps import levelset
    S = np.zeros((3, 3, 3), F32)
    with pytest.raises(ValueError):
        levelset.isosurface(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        levelset.isosurface(np.zeros((3, 0, 3)))
    with pytest.raises(TypeError):
        levelset.isosurface(S.astype(np.complex64))
    with pytest.raises(TypeError):
        levelset.isosurface(S, iso="0")
    with pytest.raises(TypeError):
        levelset.isosurface(S, iso=torch.zeros(()))
    with pytest.raises(ValueError):
        levelset.isosurface(S, origin=(0.0, 0.0))
    for bad in (0.0, -1.0, math.inf, math.nan, (1.0, 1.0), (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError):
            levelset.isosurface(S, spacing=bad)
    with pytest.raises(OverflowError):
        levelset.isosurface(np.broadcast_to(F32(0), (1024, 1024, 256)))
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    for kw in (dict(h=0.0), dict(h=-1.0), dict(h=math.nan), dict(h=0.1, field="sdf"), dict(h=0.1, pad=0), dict(h=0.1, pad=1.5),
               dict(h=0.1, beta=0.5)):
        with pytest.raises(ValueError):
            levelset.remesh_level_set(v, f, **kw)
    with pytest.raises(TypeError):
        levelset.remesh_level_set(v, f, "0.1")
    with pytest.raises(ValueError):
        levelset.remesh_level_set(v[:, :2], f, 0.1)
    with pytest.raises(TypeError):
        levelset.remesh_level_set(v, f.astype(np.float64), 0.1)


def test_cpu_tensors_raise():
    from largesteps import levelset
    with pytest.raises(RuntimeError, match="no CPU path"):
        levelset.isosurface(torch.zeros((3, 3, 3)))
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        levelset.remesh_level_set(v, f, 0.1)


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_iso_backward", "ls_iso_count", "ls_iso_fill", "ls_iso_workspace_bytes"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ls_iso_[a-z_0-9]+)\s*\(", src))) == NAMES
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert getattr(native.lib(), name).restype is ctypes.c_int
    assert sorted(n for n in native.EXPORTED_SYMBOLS if n.startswith("ls_iso_")) == NAMES
    assert native.lib().ls_version() == 110


def test_abi_argument_checks(native):
    lib = native.lib()
    E, OV, WS = native.LS_E_INVALID, native.LS_E_OVERFLOW, native.LS_E_WORKSPACE
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)                   # never dereferenced: every call below fails an argument check first
    n = ctypes.c_size_t(0)
    one, bad = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(1, 0, 1)
    nan, inf = (ctypes.c_float * 3)(1, math.nan, 1), (ctypes.c_float * 3)(math.inf, 1, 1)
    assert lib.ls_iso_workspace_bytes(4, 4, 4, None) == E
    assert lib.ls_iso_workspace_bytes(0, 4, 4, ctypes.byref(n)) == E
    assert lib.ls_iso_workspace_bytes(4, 4, -1, ctypes.byref(n)) == E
    assert lib.ls_iso_workspace_bytes(1024, 1024, 256, ctypes.byref(n)) == OV                   # 8 N = 2^31
    assert lib.ls_iso_workspace_bytes(2 ** 40, 2 ** 40, 2 ** 40, ctypes.byref(n)) == OV
    assert lib.ls_iso_workspace_bytes(1024, 1024, 255, ctypes.byref(n)) == OV                   # 12 Nc reaches 2^31 before 8 N does
    assert lib.ls_iso_workspace_bytes(2 ** 28 - 1, 1, 1, ctypes.byref(n)) == 0                  # no cubes: only the nodes count
    assert lib.ls_iso_workspace_bytes(1, 4, 4, ctypes.byref(n)) == 0 and n.value >= 16 * 9
    assert lib.ls_iso_workspace_bytes(5, 6, 7, ctypes.byref(n)) == 0 and n.value >= 210 * 9 + 120 * 8
    ws = n.value
    assert lib.ls_iso_count(None, 5, 6, 7, 0.0, x, ws, x, 0, None) == E
    assert lib.ls_iso_count(x, 5, 6, 7, 0.0, None, ws, x, 0, None) == E
    assert lib.ls_iso_count(x, 5, 6, 7, 0.0, x, ws, None, 0, None) == E
    assert lib.ls_iso_count(x, 5, 0, 7, 0.0, x, ws, x, 0, None) == E
    assert lib.ls_iso_count(x, 1024, 1024, 256, 0.0, x, ws, x, 0, None) == OV
    assert lib.ls_iso_count(x, 5, 6, 7, 0.0, x, ws - 1, x, 0, None) == WS
    assert lib.ls_iso_fill(None, 5, 6, 7, 0.0, one, one, x, ws, 1, 1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, None, one, x, ws, 1, 1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, None, x, ws, 1, 1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, None, ws, 1, 1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, 1, 1, None, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, 1, 1, x, x, None, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, -1, 1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, 1, -1, x, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 5, 6, 0, 0.0, one, one, x, ws, 1, 1, x, x, x, 0, None) == E
    for sp in (bad, nan, inf):
        assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, sp, x, ws, 1, 1, x, x, x, 0, None) == E
        assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, sp, x, ws, 1, x, x, 0, None) == E
    assert lib.ls_iso_fill(x, 1024, 1024, 256, 0.0, one, one, x, ws, 1, 1, x, x, x, 0, None) == OV
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, 2 ** 31, 1, x, x, x, 0, None) == OV
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws - 1, 1, 1, x, x, x, 0, None) == WS
    assert lib.ls_iso_fill(x, 5, 6, 7, 0.0, one, one, x, ws, 0, 0, None, None, None, 0, None) == 0          # nothing to write
    assert lib.ls_iso_fill(x, 1, 4, 4, 0.0, one, one, x, ws, 0, 0, None, None, None, 0, None) == 0          # a side of 1: valid, empty
    assert lib.ls_iso_backward(None, 5, 6, 7, 0.0, one, one, x, ws, 1, x, x, 0, None) == E
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, None, ws, 1, x, x, 0, None) == E
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, x, ws, 1, None, x, 0, None) == E
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, x, ws, 1, x, None, 0, None) == E
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, x, ws, -1, x, x, 0, None) == E
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, x, ws, 2 ** 31, x, x, 0, None) == OV
    assert lib.ls_iso_backward(x, 5, 6, 7, 0.0, one, one, x, ws - 1, 1, x, x, 0, None) == WS
