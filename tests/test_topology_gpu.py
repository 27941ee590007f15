"""
largesteps.topology on the device (csrc/topology.hip) against tests/topology_statement.py. Every result is integer-valued with one right
answer, and the statement forms the fp64 measures in the device's order, so the device must return exactly the statement's arrays: no
tolerance anywhere except the derived bound n 2^-52 sum|term| of test_topology_cpu.py, re-checked on the device's measures. The meshes
are the smallest that reach each way the kernels can go wrong: contention and deep parent chains in the hooking, more than one radix
byte, doubling past one workgroup and over a length that is no power of two, both branches of the segmented sum.
"""
import numpy as np
import pytest
import torch

import topology_statement as st

pytestmark = pytest.mark.gpu
MESHES = st.small_meshes()
_topologies = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def topology(name):
    if name not in _topologies:
        _topologies[name] = st.Topology(*MESHES[name])
    return _topologies[name]


def arr(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def same(a, b):
    """equal shapes and equal values; fp64 by its bits"""
    a, b = arr(a), arr(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        a, b = a.astype(np.float64).view(np.int64), b.astype(np.float64).view(np.int64)
    return a.shape == b.shape and np.array_equal(a, b)


def check(topo, T, dtype=None):
    """every connectivity result of a MeshTopology against the statement's Topology"""
    assert topo.num_vertex_components == T.num_vertex_components and topo.num_facet_components == T.num_facet_components
    assert same(topo.vertex_components, T.vertex_components) and same(topo.facet_components, T.facet_components)
    assert same(topo.edges, T.edges) and same(topo.edge_faces, T.edge_faces)
    assert (topo.is_edge_manifold, topo.is_oriented, topo.is_closed) == (T.is_edge_manifold, T.is_oriented, T.is_closed)
    assert all(isinstance(x, bool) for x in (topo.is_edge_manifold, topo.is_oriented, topo.is_closed))
    assert same(topo.counts(), T.counts()) and arr(topo.counts()).dtype == np.int64 and arr(topo.counts()).shape == (T.num_facet_components, 6)
    assert same(topo.euler_characteristic(), T.euler_characteristic())
    if T.loops_defined:
        loops, ptr = topo.boundary_loops()
        rl, rp = T.boundary_loops()
        assert same(loops, rl) and same(ptr, rp)
    else:
        with pytest.raises(ValueError, match="boundary is not a set of oriented cycles"):
            topo.boundary_loops()
    if dtype is not None:
        for x in (topo.vertex_components, topo.facet_components, topo.edges, topo.edge_faces):
            assert arr(x).dtype == dtype


def on(dev, F, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(F)).to(dev).to(dtype)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_largesteps_topology_exists_and_labels_two_tetrahedra(dev):
    """(fails without the feature: the module does not exist)"""
    from largesteps.topology import (MeshTopology, vertex_components, facet_components, boundary_loops, boundary_loop,      # noqa: F401
                                     is_edge_manifold, remove_unreferenced, keep_components, keep_largest_component, keep_outer_components)
    F, V = MESHES["two_tetrahedra"]
    topo = MeshTopology(on(dev, F), V)
    assert topo.num_vertex_components == 2 and topo.num_facet_components == 2
    assert topo.vertex_components.tolist() == [0] * 4 + [1] * 4 and topo.facet_components.tolist() == [0] * 4 + [1] * 4
    assert topo.vertex_components.device == dev and topo.is_closed and topo.is_oriented and topo.is_edge_manifold
    check(topo, topology("two_tetrahedra"))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int64", "int32", "numpy64", "numpy32"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_the_small_cases(dev, name, kind):
    from largesteps import topology as tp
    F, V = MESHES[name]
    T = topology(name)
    np_dtype = np.int32 if kind.endswith("32") else np.int64
    if kind.startswith("numpy"):
        Fin = F.astype(np_dtype)
    else:
        Fin = on(dev, F, torch.int32 if kind == "int32" else torch.int64)
    topo = tp.MeshTopology(Fin, V)
    check(topo, T, np_dtype)
    assert isinstance(topo.vertex_components, np.ndarray) == kind.startswith("numpy")
    # the one-shots
    vc = tp.vertex_components(Fin, V)
    assert same(vc, T.vertex_components) and arr(vc).dtype == np_dtype and isinstance(vc, np.ndarray) == kind.startswith("numpy")
    fc = tp.facet_components(Fin)
    assert same(fc, T.facet_components) and arr(fc).dtype == np_dtype
    assert tp.is_edge_manifold(Fin) == T.is_edge_manifold
    if F.shape[0]:
        assert same(tp.vertex_components(Fin), T.vertex_components[:F.max() + 1])          # V = max(F) + 1 when it is not given
    if T.loops_defined:
        got, ref = tp.boundary_loops(Fin), T.loop_list()
        assert len(got) == len(ref) and all(same(g, r) for g, r in zip(got, ref))
        longest = max(ref, key=len) if ref else np.zeros(0, dtype=np.int64)                # (max returns the first of equal lengths)
        assert same(tp.boundary_loop(Fin), longest)
    else:
        with pytest.raises(ValueError, match="boundary is not a set of oriented cycles"):
            tp.boundary_loops(Fin)


def test_what_the_table_expects(dev):
    """the expectations of the small cases, stated on the device's own results"""
    from largesteps.topology import MeshTopology
    t = {name: MeshTopology(on(dev, F), V) for name, (F, V) in MESHES.items()}
    c = t["cones_tip_to_tip"]
    assert c.num_vertex_components == 1 and c.num_facet_components == 2 and c.counts()[:, 1].tolist() == [5, 5]
    c = t["three_faces_on_an_edge"]
    assert c.num_facet_components == 1 and c.counts()[0, 4].item() == 1 and not c.is_edge_manifold
    assert t["same_direction"].counts()[0, 5].item() == 1
    c = t["moebius8"]
    assert c.counts()[0, 5].item() >= 1 and not c.is_oriented
    with pytest.raises(ValueError, match="boundary is not a set of oriented cycles"):
        c.boundary_loops()
    loops, ptr = t["plane4"].boundary_loops()
    assert ptr.tolist() == [0, 12] and loops.tolist() == [0, 1, 2, 3, 7, 11, 15, 14, 13, 12, 8, 4]
    assert t["plane6_hole"].boundary_loops()[1].shape[0] - 1 == 2
    assert t["shells2"].num_facet_components == 2 and t["shells2"].euler_characteristic().tolist() == [2, 2]
    e = t["empty"]
    assert e.num_facet_components == 0 and e.num_vertex_components == 5 and e.vertex_components.tolist() == [0, 1, 2, 3, 4]
    assert e.facet_components.shape == (0,) and e.edges.shape == (0, 2) and e.counts().shape == (0, 6)
    assert e.measures(torch.zeros((5, 3), device=dev)).shape == (0, 2)
    F2, I, J = e.keep(torch.zeros(0, dtype=torch.bool, device=dev))
    assert F2.shape == (0, 3) and I.tolist() == [-1] * 5 and J.shape == (0,)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["natural", "reversed", "random"])
def test_hooking_under_contention_and_deep_chains(dev, numbering):
    """20 000 triangles in one strip: more than one workgroup, many scan chunks, one component that every thread hooks into. Reversed
    vertex ids give the longest parent chains. The result must not depend on the interleaving: two runs, equal arrays, the statement's."""
    from largesteps.topology import MeshTopology
    F, V = st.strip(20000)
    rng = np.random.default_rng(11)
    perm = {"natural": np.arange(V), "reversed": np.arange(V)[::-1], "random": rng.permutation(V)}[numbering]
    F, V = st.renumbered(F, V, perm, rng.permutation(F.shape[0]))
    T = st.Topology(F, V)
    assert T.num_facet_components == 1 and T.num_vertex_components == 1 and len(T.loop_list()) == 1
    tf = on(dev, F)
    a, b = MeshTopology(tf, V), MeshTopology(tf, V)
    check(a, T)
    check(b, T)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def test_more_than_one_radix_byte_and_many_components(dev):
    from largesteps.topology import MeshTopology
    V = 70000
    rng = np.random.default_rng(12)
    ids = 65537 + rng.permutation(V - 65537)[:3000]
    F = ids.reshape(1000, 3).astype(np.int64)
    T = st.Topology(F, V)
    assert T.num_vertex_components == 68000 and T.num_facet_components == 1000
    check(MeshTopology(on(dev, F), V), T)
    check(MeshTopology(on(dev, F, torch.int32), V), T)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("holes", [0, 5])
def test_doubling_past_one_workgroup(dev, holes):
    """plane(300) under a seeded renumbering: one loop of 1 196 vertices (no power of two, more than one workgroup), and with a 3 x 3 block
    of cells removed at five places six loops"""
    from largesteps.topology import MeshTopology
    n = 300
    at = [(20, 30), (150, 150), (250, 40), (60, 260), (270, 270)][:holes]
    F, V = st.without_cells(n, [(x + i, y + j) for x, y in at for i in range(3) for j in range(3)])
    F, V = st.renumbered(F, V, np.random.default_rng(13).permutation(V))
    T = st.Topology(F, V)
    lens = sorted(len(l) for l in T.loop_list())
    assert lens == [12] * holes + [1196]
    check(MeshTopology(on(dev, F), V), T)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_measures_bit_for_bit(dev):
    from largesteps.topology import MeshTopology
    V, F = st.hollow_ball(3)
    T = st.Topology(F, V.shape[0])
    ref = st.measures(T, V)
    assert T.num_facet_components == 2 and T.counts()[:, 0].tolist() == [180, 180]          # above 64 faces: the wave's order
    topo = MeshTopology(on(dev, F), V.shape[0])
    tv = torch.from_numpy(V).to(dev)
    got = topo.measures(tv)
    print("hollow ball: areas", arr(got)[:, 0], "volumes", arr(got)[:, 1])
    assert got.dtype == torch.float64 and got.device == dev and same(got, ref)
    assert same(topo.measures(tv), got)                                                    # a second call: the same bits
    assert same(topo.measures(V), ref) and isinstance(topo.measures(V), np.ndarray)
    g = arr(got)
    # a sanity line, to the discretisation only: inscribed polyhedra of radius 1 and 1/2, the inner one facing inward
    assert 0.9 < g[0, 0] / (4 * np.pi) < 1 and 0.9 < g[1, 0] / np.pi < 1 and 0.85 < g[0, 1] / (4 * np.pi / 3) < 1 and 0.85 < g[1, 1] / (-np.pi / 6) < 1
    # the derived bound of test_topology_cpu.py on the device's result: any order of an n-term fp64 sum
    terms = st.face_terms(V, F)
    for k in range(2):
        t = terms[T.facet_components == k]
        assert (np.abs(g[k] - np.sum(t, axis=0)) <= t.shape[0] * 2.0 ** -52 * np.abs(t).sum(0)).all()
    # components of 4 faces: the one-thread order
    F4, V4 = st.tetrahedra(50)
    X = st.positions(V4, 3)
    T4 = st.Topology(F4, V4)
    assert same(MeshTopology(on(dev, F4, torch.int32), V4).measures(torch.from_numpy(X).to(dev)), st.measures(T4, X))
    with pytest.raises(RuntimeError, match="not differentiable"):
        topo.measures(tv.clone().requires_grad_())


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def three_pieces():
    """a fine small sphere (most faces), a large sheet in the plane z = 0 (most area, every volume term zero), a coarse large sphere
    (most volume), and vertices in no face before, between and after"""
    from largesteps import synthetic
    v0, f0 = synthetic.icosphere(3)
    v1, f1 = synthetic.plane(4)
    v2, f2 = synthetic.icosphere(1)
    pad = np.full((2, 3), 9.0, dtype=np.float32)
    V = np.concatenate([pad, 0.1 * v0, pad, 20.0 * v1 * np.array([1, 1, 0], dtype=np.float32), 2.0 * v2 - 7.0, pad]).astype(np.float32)
    o1 = 2 + v0.shape[0] + 2
    F = np.concatenate([f0 + 2, f1 + o1, f2 + o1 + v1.shape[0]]).astype(np.int64)
    return V, F


@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_keep_and_the_component_filters(dev, idx):
    from largesteps import topology as tp
    V, F = three_pieces()
    T = st.Topology(F, V.shape[0])
    assert T.num_facet_components == 3
    tv, tf = torch.from_numpy(V).to(dev), on(dev, F, idx)
    topo = tp.MeshTopology(tf, V.shape[0])
    for mask in ([True, False, True], [False, True, False], [True, True, True], [False, False, False]):
        F2, I, J = topo.keep(torch.tensor(mask, device=dev))
        rF, rI, rJ = T.keep(mask)
        assert same(F2, rF) and same(I, rI) and same(J, rJ) and F2.dtype == idx and I.dtype == idx and J.dtype == idx
        assert same(I[J.long()], np.arange(J.shape[0]))
        V2, F2b = tp.keep_components(tv, tf, torch.tensor(mask, device=dev))
        assert same(F2b, rF) and np.array_equal(arr(V2).view(np.int32), V[rJ].view(np.int32))
        F2n, In, Jn = topo.keep(np.array(mask))                   # a numpy mask on a tensor handle
        assert same(F2n, rF) and same(In, rI) and same(Jn, rJ)
    NV, NF, I, J = tp.remove_unreferenced(tv, tf)
    rF, rI, rJ = T.keep([True] * 3)
    assert same(NF, rF) and same(I, rI) and same(J, rJ) and np.array_equal(arr(NV).view(np.int32), V[rJ].view(np.int32))
    assert (arr(I)[[0, 1, -1, -2]] == -1).all() and same(arr(I)[F], rF)
    NVn, NFn, In, Jn = tp.remove_unreferenced(V, F.astype(np.int32 if idx == torch.int32 else np.int64))      # numpy in, numpy out
    assert all(isinstance(x, np.ndarray) for x in (NVn, NFn, In, Jn)) and same(NFn, rF) and np.array_equal(NVn.view(np.int32), V[rJ].view(np.int32))
    picks = []
    for by in ("faces", "area", "volume"):
        mask = st.largest(T, V, by)
        picks.append(int(np.argmax(mask)))
        V2, F2 = tp.keep_largest_component(tv, tf, by=by)
        rF, _, rJ = T.keep(mask)
        assert same(F2, rF) and np.array_equal(arr(V2).view(np.int32), V[rJ].view(np.int32))
    assert picks == [0, 1, 2]                                     # the three choices differ
    with pytest.raises(ValueError, match="by must be"):
        tp.keep_largest_component(tv, tf, by="edges")


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere2", "plane4"])
def test_edges_are_the_subdivision_s(dev, name):
    from largesteps.subdivide import Subdivision
    from largesteps.topology import MeshTopology
    F, V = MESHES[name]
    tf = on(dev, F)
    assert torch.equal(MeshTopology(tf, V).edges, Subdivision(tf, V).edges[0])


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
def test_measures_and_keep_replay_in_a_captured_graph(dev):
    from largesteps.topology import MeshTopology
    V, F = three_pieces()
    tv, tf = torch.from_numpy(V).to(dev), on(dev, F)
    mask = torch.tensor([True, False, True], device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        topo = MeshTopology(tf, V.shape[0])                      # the constructor synchronises: eager, on the stream of the capture
        eager_m = topo.measures(tv).clone()
        eager_k = [x.clone() for x in topo.keep(mask)]
        sizes = (eager_k[0].shape[0], eager_k[2].shape[0])           # read back once, eagerly: a capture cannot
        assert all(same(a, b) for a, b in zip(topo.keep(mask, sizes=sizes), eager_k))
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                 # one plain sequential graph
        m = topo.measures(tv)
        k = topo.keep(mask, sizes=sizes)
    m.zero_()
    for x in k:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert same(m, eager_m) and all(same(a, b) for a, b in zip(k, eager_k))


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    from largesteps import topology as tp
    F, V = MESHES["tetrahedron"]
    with pytest.raises(RuntimeError, match="HIP device"):
        tp.MeshTopology(torch.from_numpy(F), V)                                      # a CPU tensor
    with pytest.raises(TypeError, match="int32 or int64"):
        tp.MeshTopology(on(dev, F).float(), V)
    with pytest.raises(TypeError):
        tp.MeshTopology(F.astype(np.float64), V)
    for bad in (4, -1):
        G = F.copy()
        G[2, 1] = bad
        with pytest.raises(ValueError, match=r"a face index is outside \[0, 4\)"):
            tp.MeshTopology(on(dev, G), V)
    G = F.copy()
    G[1] = [0, 3, 3]
    with pytest.raises(ValueError, match="a face names a vertex twice"):
        tp.MeshTopology(on(dev, G), V)
    topo = tp.MeshTopology(on(dev, F), V)
    with pytest.raises(ValueError, match="mask must be"):
        topo.keep(torch.ones(2, dtype=torch.bool, device=dev))
    with pytest.raises(TypeError, match="mask must be bool"):
        topo.keep(torch.ones(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="rows"):
        topo.measures(torch.zeros((5, 3), device=dev))
    with pytest.raises(ValueError):
        tp.MeshTopology(on(dev, F), -1)
    with pytest.raises(OverflowError):
        tp.MeshTopology(on(dev, F), 1 << 31)


# ---- 11 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_outer_skin_of_a_level_set(dev):
    """remesh_level_set returns every closed sheet (its signature is pinned by tests/test_isosurf_cpu.py and stays as it is); the filters
    of largesteps.topology take the shell around the void away, on the device, and remesh_botsch accepts what is left"""
    from largesteps.levelset import remesh_level_set
    from largesteps.remesh import remesh_botsch
    from largesteps.topology import MeshTopology, keep_largest_component, keep_outer_components
    V, F = st.hollow_ball(3)
    tv, tf = torch.from_numpy(V).to(dev), on(dev, F)
    Va, Fa = remesh_level_set(tv, tf, 0.1)
    every = MeshTopology(Fa, Va.shape[0])
    assert every.num_facet_components == 2 and (arr(every.measures(Va))[:, 1] > 0).sum() == 1          # the skin and the shell of the void
    Vo, Fo = keep_outer_components(Va, Fa)
    topo = MeshTopology(Fo, Vo.shape[0])
    assert topo.num_facet_components == 1 and topo.num_vertex_components == 1 and topo.is_closed and topo.is_oriented
    assert topo.euler_characteristic().tolist() == [2] and arr(topo.measures(Vo))[0, 1] > 0
    T = st.Topology(arr(Fa), Va.shape[0])                          # and it is the statement's filter
    rF, _, rJ = T.keep(st.measures(T, arr(Va))[:, 1] > 0)
    assert same(Fo, rF) and np.array_equal(arr(Vo).view(np.int32), arr(Va)[rJ].view(np.int32))
    Vl, Fl = keep_largest_component(Va, Fa, by="volume")
    assert torch.equal(Fl, Fo) and torch.equal(Vl.view(torch.int32), Vo.view(torch.int32))
    V3, F3 = remesh_botsch(Vo, Fo, 1, 0.15, True)
    assert F3.shape[0] > 0 and F3.shape[1] == 3 and torch.isfinite(V3).all()
