"""
tests/topology_statement.py checked against what it shares nothing with -- scipy's connected components, the Euler characteristics of
known surfaces, hand-written loops, numpy's own sum -- and the ctypes table of ls_topo_* against the header. No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import topology_statement as st
from largesteps import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = st.small_meshes()


def by_first_appearance(labels):
    seen = {}
    return np.array([seen.setdefault(int(x), len(seen)) for x in labels], dtype=np.int64)


def scipy_components(pairs, n):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    A = sp.coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    k, labels = connected_components(A, directed=False)
    return k, by_first_appearance(labels)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_component_labels_equal_scipy(name):
    F, V = MESHES[name]
    T = st.Topology(F, V)
    k, labels = scipy_components(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), V)
    assert T.num_vertex_components == k and np.array_equal(by_first_appearance(T.vertex_components), labels)
    assert np.array_equal(by_first_appearance(T.vertex_components), T.vertex_components)       # numbered by lowest member already
    # faces that share an edge, from a dictionary of its own: every pair of faces on one unordered vertex pair
    on = {}
    for f, face in enumerate(F):
        for e in range(3):
            on.setdefault(frozenset((int(face[e]), int(face[(e + 1) % 3]))), []).append(f)
    pairs = [(g[0], h) for g in on.values() for h in g[1:]]
    k, labels = scipy_components(pairs, F.shape[0])
    assert T.num_facet_components == k and np.array_equal(by_first_appearance(T.facet_components), labels)
    assert np.array_equal(by_first_appearance(T.facet_components), T.facet_components)


def test_euler_characteristics_of_known_surfaces():
    ico = synthetic.icosphere(3)
    plane = synthetic.plane(5)
    for (F, V), chi in (((ico[1], ico[0].shape[0]), 2), ((plane[1], plane[0].shape[0]), 1), (st.torus(), 0), (st.moebius(8), 0)):
        T = st.Topology(F, V)
        assert T.num_facet_components == 1 and T.euler_characteristic().tolist() == [chi]


def test_the_table_of_small_cases():
    T = {name: st.Topology(*MESHES[name]) for name in MESHES}
    t = T["tetrahedron"]
    assert t.is_closed and t.is_oriented and t.is_edge_manifold and t.counts().tolist() == [[4, 4, 6, 0, 0, 0]]
    t = T["two_tetrahedra"]
    assert t.vertex_components.tolist() == [0] * 4 + [1] * 4 and t.facet_components.tolist() == [0] * 4 + [1] * 4
    t = T["cones_tip_to_tip"]
    assert t.num_vertex_components == 1 and t.num_facet_components == 2 and t.counts()[:, 1].tolist() == [5, 5]
    assert [l.tolist() for l in t.loop_list()] == [[1, 2, 3, 4], [5, 8, 7, 6]]
    t = T["three_faces_on_an_edge"]
    assert t.num_facet_components == 1 and t.num_nonmanifold_edges == 1 and not t.is_edge_manifold and not t.is_oriented
    assert t.edge_faces[0].tolist() == [0, 1]
    t = T["same_direction"]
    assert t.num_misoriented_edges == 1 and t.is_edge_manifold and not t.is_oriented
    t = T["moebius8"]
    assert t.num_misoriented_edges >= 1 and not t.is_oriented and t.is_edge_manifold
    with pytest.raises(ValueError, match="oriented cycles"):
        t.boundary_loops()
    t = T["plane4"]
    assert [l.tolist() for l in t.loop_list()] == [[0, 1, 2, 3, 7, 11, 15, 14, 13, 12, 8, 4]]
    t = T["plane6_hole"]
    assert [len(l) for l in t.loop_list()] == [20, 4] and t.loop_list()[1].tolist() == [14, 20, 21, 15]
    t = T["shells2"]
    assert t.num_facet_components == 2 and t.num_vertex_components == 2 and t.euler_characteristic().tolist() == [2, 2]
    t = T["unreferenced"]
    assert t.num_vertex_components == 8 and t.num_facet_components == 2
    F2, I, J = t.keep(np.array([True, True]))
    assert J.tolist() == [2, 3, 5, 6, 8, 9, 10] and I.tolist() == [-1, -1, 0, 1, -1, 2, 3, -1, 4, 5, 6, -1, -1]
    assert F2.tolist() == [[0, 1, 2], [0, 2, 3], [5, 6, 4]]
    with pytest.raises(ValueError, match="oriented cycles"):
        T["bowtie"].boundary_loops()
    t = T["empty"]
    assert t.num_facet_components == 0 and t.num_vertex_components == 5 and t.counts().shape == (0, 6) and t.is_closed
    assert [a.tolist() for a in t.boundary_loops()] == [[], [0]]


def test_edges_are_those_of_the_subdivision_statement():
    import subdiv_statement as sd
    for name in ("icosphere2", "plane4"):
        F, V = MESHES[name]
        assert np.array_equal(st.Topology(F, V).edges, sd.Topology(F, V).edges)


def test_measures_are_within_the_bound_of_any_summation_order():
    """An n-term fp64 sum in any order is within (n - 1) u sum|term| (1 + O(n u)) of the exact sum, u = 2^-53; two orders differ by at
    most twice that, which n 2^-52 sum|term| covers."""
    v, f = synthetic.icosphere(3)
    T = st.Topology(f, v.shape[0])
    got = st.measures(T, v)
    terms = st.face_terms(v, f)
    n = terms.shape[0]
    assert n == 180 and got.shape == (1, 2)
    bound = n * 2.0 ** -52 * np.abs(terms).sum(0)
    assert (np.abs(got[0] - np.sum(terms, axis=0)) <= bound).all()
    # a sphere to its discretisation: an inscribed polyhedron of 180 faces has a little less area and volume
    assert 0.9 * 4 * np.pi < got[0, 0] < 4 * np.pi and 0.85 * 4 * np.pi / 3 < got[0, 1] < 4 * np.pi / 3
    # both branches of the order: the same terms below and above 64
    acc = np.zeros(2)
    for t in terms[:64]:
        acc = acc + t
    assert np.array_equal(st.seg_sum(terms[:64]), acc)


def test_largest_component_choices_differ():
    V, F, _ = _three_pieces()
    T = st.Topology(F, V.shape[0])
    picks = [int(np.argmax(st.largest(T, V, by))) for by in ("faces", "area", "volume")]
    assert sorted(picks) == [0, 1, 2]


def _three_pieces():
    """a fine small sphere (most faces), a large flat sheet in the plane z = 0 (most area, volume terms all zero), a coarse large sphere (most volume)"""
    v0, f0 = synthetic.icosphere(3)
    v1, f1 = synthetic.plane(4)
    v2, f2 = synthetic.icosphere(1)
    V = np.concatenate([0.1 * v0, 20.0 * v1 * np.array([1, 1, 0], dtype=np.float32), 2.0 * v2 - 7.0]).astype(np.float32)
    F = np.concatenate([f0, f1 + v0.shape[0], f2 + v0.shape[0] + v1.shape[0]]).astype(np.int64)
    return V, F, (f0.shape[0], f1.shape[0], f2.shape[0])


C_TYPES = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "size_t": ctypes.c_size_t}


def test_ctypes_signatures_match_the_header():
    from largesteps import _native
    src = open(os.path.join(ROOT, "include", "largesteps_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(ls_topo_[a-z_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(decls) == ["ls_topo_build", "ls_topo_counts", "ls_topo_keep", "ls_topo_keep_workspace_bytes", "ls_topo_measures",
                             "ls_topo_workspace_bytes"]
    for name, params in decls.items():
        res, args = _native._SIGNATURES[name]
        params = [" ".join(p.split()) for p in params.split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, p)
                if issubclass(a, ctypes._Pointer):          # a typed host pointer: its target is the declared type (or an array of it)
                    base = p.replace("const ", "").split("*")[0].strip()
                    target = a._type_
                    if issubclass(target, ctypes.Array):
                        target = target._type_
                    assert target is C_TYPES[base], (name, p)
            else:
                assert a is C_TYPES[p.rsplit(" ", 1)[0]], (name, p)
