"""
The subdivision rule without a device: tests/subdiv_statement.py (the numpy restatement the device is held to, bit for bit, by
tests/test_subdiv_gpu.py) against a dense S built from a dict of edges that shares nothing with the statement's walk; the properties a
Loop / midpoint level must have (partition of unity, affine precision, the regular stencil, counts, Euler characteristic, closedness,
boundary loops); and the argument checks of the ls_subdiv_* entry points and of largesteps.subdivide, which all fail before any device
work. Bounds: a row of S X is a sum of at most n + 1 <= 201 fp64 products rounded to fp32 once, the dense product adds the same terms in
another order, so they differ by well under 8 * 2^-24 * sum |terms|.
"""
import ctypes

import numpy as np
import pytest
import torch

import subdiv_statement as st

F32 = np.float32
EPS = 2.0 ** -24
SCHEMES = (st.LOOP, st.MIDPOINT)
MESHES = st.small_meshes()
MESHES["fan200"] = st.fan(200)                              # the walk of more than 64 corners


@pytest.fixture(scope="module")
def native():
    import os
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


@pytest.fixture(scope="module")
def topologies():
    return {name: st.Topology(F, V) for name, (F, V) in MESHES.items()}


def edge_counts(F):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def boundary_loops(F):
    """the number of cycles of the boundary edges (every boundary vertex of a manifold mesh has two of them)"""
    e, cnt = edge_counts(F)
    nxt = {}
    for a, b in e[cnt == 1]:
        nxt.setdefault(int(a), []).append(int(b))
        nxt.setdefault(int(b), []).append(int(a))
    seen, loops = set(), 0
    for s in nxt:
        if s in seen:
            continue
        loops += 1
        stack = [s]
        while stack:
            v = stack.pop()
            if v not in seen:
                seen.add(v)
                stack += nxt[v]
    return loops


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_statement_against_the_dense_matrix_forward_and_backward(topologies, name, scheme):
    F, V = MESHES[name]
    T = topologies[name]
    S = st.dense_matrix(F, V, scheme)
    assert S.shape == (V + T.E, V)
    for C in (1, 3):
        X = st.values(V, C, 7 + C)
        got = st.apply(T, X, scheme)
        assert got.dtype == F32 and got.shape == (V + T.E, C)
        bound = 8 * EPS * (np.abs(S) @ np.abs(X.astype(np.float64)))
        assert (np.abs(got - S @ X.astype(np.float64)) <= bound).all()
        g = st.values(V + T.E, C, 11 + C)
        back = st.apply_transposed(T, g, scheme)
        assert back.dtype == F32 and back.shape == (V, C)
        bound = 8 * EPS * (np.abs(S.T) @ np.abs(g.astype(np.float64)))
        assert (np.abs(back - S.T @ g.astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_partition_of_unity(name, scheme):
    S = st.dense_matrix(*MESHES[name], scheme)
    assert (np.abs(S.sum(axis=1) - 1.0) <= 2.0 ** -50).all()
    assert (S >= 0.0).all()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", ["icosphere2", "plane4", "two_triangles", "unreferenced", "fan200"])
def test_affine_precision(topologies, name, scheme):
    F, V = MESHES[name]
    T = topologies[name]
    rng = np.random.default_rng(3)
    X = st.values(V, 3, 5)
    A, t = rng.standard_normal((3, 3)), rng.standard_normal(3)
    Y = (X.astype(np.float64) @ A + t).astype(F32)
    lhs = st.apply(T, Y, scheme).astype(np.float64)
    rhs = st.apply(T, X, scheme).astype(np.float64) @ A + t
    scale = max(np.abs(lhs).max(), np.abs(rhs).max(), np.abs(X).max() * np.abs(A).sum(axis=0).max() + np.abs(t).max())
    assert np.abs(lhs - rhs).max() <= 16 * EPS * scale


def test_regular_valence_six_stencil(topologies):
    F, V = MESHES["plane4"]
    S = st.dense_matrix(F, V, st.LOOP)
    T = topologies["plane4"]
    regular = [v for v in range(V) if T.valence[v] == 6 and not T.bflag[v]]
    assert regular == [5, 6, 9, 10]
    for v in regular:
        row = S[v]
        assert row[v] == 10.0 / 16.0
        nb = np.flatnonzero(row)
        assert len(nb) == 7 and all(row[u] == 1.0 / 16.0 for u in nb if u != v)
        e = np.zeros((V, 1), F32)                            # and the statement applies that row
        e[v] = 1.0
        assert st.apply(T, e, st.LOOP)[v, 0] == F32(10.0 / 16.0)
    tet = st.dense_matrix(*MESHES["tetrahedron"], st.LOOP)   # valence 3: beta = 3 / 16
    assert tet[0, 0] == 1.0 - 9.0 / 16.0 and tet[0, 1] == 3.0 / 16.0


@pytest.mark.parametrize("name", sorted(MESHES))
def test_counts_euler_characteristic_and_boundaries(topologies, name):
    F, V = MESHES[name]
    T = topologies[name]
    e, cnt = edge_counts(F)
    assert T.E == len(e) and T.faces.shape == (4 * len(F), 3)
    assert np.array_equal(T.edges[np.lexsort((T.edges[:, 1], T.edges[:, 0]))], e)
    V1 = V + T.E
    assert T.faces.min() >= 0 and T.faces.max() == V1 - 1
    e1, cnt1 = edge_counts(T.faces)
    assert cnt1.max() <= 2
    assert V - len(e) + len(F) == V1 - len(e1) + len(T.faces)                 # Euler characteristic (unreferenced vertices on both sides)
    assert len(e1) == 2 * len(e) + 3 * len(F)
    if (cnt == 2).all():
        assert (cnt1 == 2).all()                                              # closed in, closed out
    assert (cnt1 == 1).sum() == 2 * (cnt == 1).sum()
    assert boundary_loops(T.faces) == boundary_loops(F)
    T2 = st.Topology(T.faces, V1)                                             # the fine mesh is a valid input again
    assert T2.E == len(e1)


def test_levels_compose():
    F, V = MESHES["two_triangles"]
    X = st.values(V, 3, 1)
    X2, F2 = st.subdivide(F, V, X, st.LOOP, 2)
    X1, F1 = st.subdivide(F, V, X, st.LOOP, 1)
    X2b, F2b = st.subdivide(F1, X1.shape[0], X1, st.LOOP, 1)
    assert np.array_equal(X2.view(np.int32), X2b.view(np.int32)) and np.array_equal(F2, F2b)
    assert F2.shape[0] == 16 * len(F)


def test_the_statement_refuses_what_the_constructor_refuses():
    three = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    bowtie = np.array([[0, 1, 2], [0, 3, 4]])
    with pytest.raises(ValueError, match="non-manifold edge"):
        st.Topology(three, 5)
    with pytest.raises(ValueError, match="non-manifold vertex"):
        st.Topology(bowtie, 5)
    with pytest.raises(ValueError):
        st.Topology(np.array([[0, 1, 1]]), 3)
    with pytest.raises(ValueError):
        st.Topology(np.array([[0, 1, 3]]), 3)


NAMES = ["ls_subdiv_apply", "ls_subdiv_apply_backward", "ls_subdiv_topology", "ls_subdiv_workspace_bytes"]


def test_symbols_are_bound(native):
    assert sorted(n for n in native.EXPORTED_SYMBOLS if n.startswith("ls_subdiv_")) == NAMES
    assert native.lib().ls_version() == 110


def test_abi_argument_checks(native):
    lib = native.lib()
    E, OV, WS = native.LS_E_INVALID, native.LS_E_OVERFLOW, native.LS_E_WORKSPACE
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)                   # never dereferenced: every call below fails an argument check first
    n = ctypes.c_size_t(0)
    assert lib.ls_subdiv_workspace_bytes(4, 4, None) == E
    assert lib.ls_subdiv_workspace_bytes(-1, 4, ctypes.byref(n)) == E
    assert lib.ls_subdiv_workspace_bytes(4, -1, ctypes.byref(n)) == E
    assert lib.ls_subdiv_workspace_bytes((2 ** 31 + 11) // 12, 4, ctypes.byref(n)) == OV            # 12 F reaches 2^31
    assert lib.ls_subdiv_workspace_bytes(4, 2 ** 31, ctypes.byref(n)) == OV
    assert lib.ls_subdiv_workspace_bytes(0, 0, ctypes.byref(n)) == 0
    assert lib.ls_subdiv_workspace_bytes(20, 12, ctypes.byref(n)) == 0 and n.value >= 4 * (13 + 4 * 60 + 1 + 3 * 60)
    ws = n.value
    hE, hs = ctypes.c_int64(0), ctypes.c_int(0)
    e, s = ctypes.byref(hE), ctypes.byref(hs)

    def topo(faces=x, idx=8, F=20, V=12, out=(x,) * 10, hE=e, hs=s, w=x, wb=ws):
        return lib.ls_subdiv_topology(faces, idx, F, V, *out, hE, hs, w, wb, 0, None)

    assert topo(faces=None) == E and topo(idx=2) == E and topo(F=-1) == E and topo(V=-1) == E
    assert topo(hE=None) == E and topo(hs=None) == E and topo(w=None) == E
    for k in range(10):
        assert topo(out=tuple(None if j == k else x for j in range(10))) == E, k
    assert topo(F=(2 ** 31 + 11) // 12) == OV and topo(V=2 ** 31) == OV
    assert topo(wb=ws - 1) == WS
    assert "workspace too small" in native.last_error()

    for fn in (lib.ls_subdiv_apply, lib.ls_subdiv_apply_backward):
        def run(X=x, F=20, V=12, E_=30, C=3, scheme=1, arrays=(x,) * 9, out=x):
            return fn(X, F, V, E_, C, scheme, *arrays, out, 0, None)

        assert run(X=None) == E and run(out=None) == E
        for k in range(9):
            assert run(arrays=tuple(None if j == k else x for j in range(9))) == E, k
        assert run(F=-1) == E and run(V=-1) == E and run(E_=-1) == E and run(E_=61) == E
        assert run(C=0) == E and run(C=33) == E and run(scheme=2) == E and run(scheme=-1) == E
        assert run(F=(2 ** 31 + 11) // 12, E_=1) == OV
        assert run(F=10 ** 8, V=2 ** 31 - 10, E_=10) == OV                                     # V + E reaches 2^31
    assert lib.ls_subdiv_apply(None, 0, 0, 0, 3, 1, *(None,) * 9, None, 0, None) == 0               # nothing to do


def test_python_argument_checks_need_no_device():
    from largesteps import subdivide
    F = np.array([[0, 1, 2]], np.int64)
    V = np.zeros((3, 3), F32)
    for bad in (F[:, :2], F.reshape(-1), np.zeros((1, 3, 1), np.int64)):
        with pytest.raises(ValueError):
            subdivide.Subdivision(bad, 3)
    with pytest.raises(TypeError):
        subdivide.Subdivision(F.astype(np.float32), 3)
    with pytest.raises(TypeError):
        subdivide.Subdivision(F, 3.0)
    with pytest.raises(TypeError):
        subdivide.Subdivision(F, 3, levels=1.0)
    with pytest.raises(TypeError):
        subdivide.Subdivision(F, 3, levels=True)
    with pytest.raises(TypeError):
        subdivide.Subdivision(F, 3, scheme=1)
    with pytest.raises(ValueError):
        subdivide.Subdivision(F, 3, scheme="catmull-clark")
    with pytest.raises(ValueError):
        subdivide.Subdivision(F, 3, levels=-1)
    with pytest.raises(ValueError):
        subdivide.Subdivision(F, -3)
    with pytest.raises(OverflowError):
        subdivide.Subdivision(F, 3, levels=15)               # 12 * 4^14 reaches 2^31 at the last level
    with pytest.raises(OverflowError):
        subdivide.loop(V, F, 15)
    with pytest.raises(OverflowError):
        subdivide.Subdivision(F, 2 ** 31, levels=1)
    with pytest.raises(RuntimeError, match="HIP device"):                     # CPU tensors raise
        subdivide.Subdivision(torch.from_numpy(F), 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        subdivide.loop(torch.from_numpy(V), torch.from_numpy(F))
    with pytest.raises(ValueError):
        subdivide.upsample(V[:, :2], F)
    with pytest.raises(TypeError):
        subdivide.upsample(V.astype(np.complex64), F)
    with pytest.raises(TypeError):
        subdivide.loop(V, F, number_of_subdivs="1")
