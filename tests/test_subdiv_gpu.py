"""
largesteps.subdivide on the device (csrc/subdiv.hip) against tests/subdiv_statement.py. The statement numbers edges and faces by the
device's rule and forms every fp64 sum in the device's order, so the device must return exactly the statement's arrays: faces, edges,
S X and S^T g, bit for bit, no tolerance anywhere. The meshes are the smallest that reach every branch of the rule (valences 3, 4, 5
and 6, all-boundary, boundary vertices with an interior edge, mixed, inconsistent winding, an unreferenced vertex).
"""
import numpy as np
import pytest
import torch

import subdiv_statement as st

pytestmark = pytest.mark.gpu
F32 = np.float32
SCHEMES = (st.LOOP, st.MIDPOINT)
MESHES = st.small_meshes()
_topologies = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def topology(name):
    if name not in _topologies:
        _topologies[name] = st.Topology(*MESHES[name])
    return _topologies[name]


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def check(dev, F, V, T, scheme, C=3, idx=torch.int64, seed=0):
    """faces, edges, S X and S^T g of a one-level handle against the statement"""
    from largesteps.subdivide import Subdivision
    tf = torch.from_numpy(F).to(dev).to(idx)
    sub = Subdivision(tf, V, scheme=scheme)
    assert sub.num_vertices == V + T.E and sub.faces.dtype == idx and sub.faces.device == tf.device
    assert same(sub.faces.to(torch.int64), T.faces)
    assert len(sub.edges) == 1 and sub.edges[0].dtype == idx and same(sub.edges[0].to(torch.int64), T.edges)
    x, g = st.values(V, C, seed), st.values(V + T.E, C, seed + 1)
    X = torch.from_numpy(x).to(dev).requires_grad_()
    Y = sub.apply(X)
    assert Y.dtype == torch.float32 and Y.shape == (V + T.E, C) and Y.requires_grad
    assert same(Y, st.apply(T, x, scheme))
    gX, = torch.autograd.grad(Y, X, torch.from_numpy(g).to(dev))
    assert same(gX, st.apply_transposed(T, g, scheme))
    return sub


def test_largesteps_subdivide_exists_and_refines_a_tetrahedron(dev):
    """(fails without the feature: the module does not exist)"""
    from largesteps.subdivide import Subdivision, loop, upsample     # noqa: F401
    F, V = MESHES["tetrahedron"]
    sub = check(dev, F, V, topology("tetrahedron"), st.LOOP)
    assert sub.num_vertices == 10 and sub.faces.shape == (16, 3)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_branch_bit_for_bit(dev, name, scheme):
    F, V = MESHES[name]
    check(dev, F, V, topology(name), scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("C", [1, 3, 5, 32])
def test_channel_counts_and_int32_faces(dev, C, scheme):
    for name in ("icosphere2", "plane4"):
        F, V = MESHES[name]
        check(dev, F, V, topology(name), scheme, C=C, idx=torch.int32, seed=C)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_a_non_contiguous_x(dev, scheme):
    from largesteps.subdivide import Subdivision
    F, V = MESHES["plane4"]
    T = topology("plane4")
    wide = st.values(V, 6, 3)
    g = st.values(V + T.E, 3, 4)
    W = torch.from_numpy(wide).to(dev).requires_grad_()
    X = W[:, ::2]
    assert not X.is_contiguous()
    sub = Subdivision(torch.from_numpy(F).to(dev), V, scheme=scheme)
    Y = sub.apply(X)
    assert same(Y, st.apply(T, np.ascontiguousarray(wide[:, ::2]), scheme))
    gW, = torch.autograd.grad(Y, W, torch.from_numpy(g).to(dev))
    ref = np.zeros_like(wide)
    ref[:, ::2] = st.apply_transposed(T, g, scheme)
    assert same(gW, ref)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_three_levels_equal_three_handles_chained_and_the_statement(dev, scheme):
    from largesteps.subdivide import Subdivision
    F, V = MESHES["two_triangles"]
    tf = torch.from_numpy(F).to(dev)
    x = st.values(V, 3, 9)
    sub = Subdivision(tf, V, scheme=scheme, levels=3)
    X = torch.from_numpy(x).to(dev).requires_grad_()
    Y = sub.apply(X)
    Xc = torch.from_numpy(x).to(dev).requires_grad_()
    y, f, nv, edges = Xc, tf, V, []
    for _ in range(3):
        h = Subdivision(f, nv, scheme=scheme)
        y, f, nv = h.apply(y), h.faces, h.num_vertices
        edges += h.edges
    assert same(Y, y) and same(sub.faces, f) and sub.num_vertices == nv and sub.faces.shape[0] == 64 * len(F)
    assert len(sub.edges) == 3 and all(same(a, b) for a, b in zip(sub.edges, edges))
    g = torch.from_numpy(st.values(nv, 3, 10)).to(dev)
    assert same(torch.autograd.grad(Y, X, g)[0], torch.autograd.grad(y, Xc, g)[0])
    ys, fs = st.subdivide(F, V, x, scheme, 3)
    assert same(Y, ys) and same(sub.faces, fs)
    gs = g.cpu().numpy()
    for T in reversed(st.levels_of(F, V, 3)):
        gs = st.apply_transposed(T, gs, scheme)
    assert same(torch.autograd.grad(Y, X, g)[0], gs)


def test_zero_levels_are_the_identity(dev):
    from largesteps.subdivide import Subdivision, loop
    F, V = MESHES["octahedron"]
    tf = torch.from_numpy(F).to(dev)
    sub = Subdivision(tf, V, levels=0)
    X = torch.from_numpy(st.values(V, 3, 0)).to(dev)
    assert sub.faces is tf and sub.apply(X) is X and sub.num_vertices == V and sub.edges == []
    NV, NF = loop(X, tf, 0)
    assert NV is X and same(NF, F)


def test_an_empty_mesh_and_a_mesh_without_faces(dev):
    from largesteps.subdivide import Subdivision
    sub = Subdivision(torch.zeros((0, 3), dtype=torch.int64, device=dev), 5)
    X = torch.from_numpy(st.values(5, 3, 0)).to(dev).requires_grad_()
    Y = sub.apply(X)
    assert sub.faces.shape == (0, 3) and sub.num_vertices == 5 and same(Y, X)
    g = torch.from_numpy(st.values(5, 3, 1)).to(dev)
    assert same(torch.autograd.grad(Y, X, g)[0], g)


def test_meshes_the_constructor_refuses(dev):
    from largesteps.subdivide import Subdivision

    def build(F, V, **kw):
        return Subdivision(torch.tensor(F, dtype=torch.int64, device=dev), V, **kw)
    with pytest.raises(ValueError, match="non-manifold edge"):
        build([[0, 1, 2], [0, 1, 3], [0, 1, 4]], 5)                          # three faces on one edge
    with pytest.raises(ValueError, match="non-manifold vertex"):
        build([[0, 1, 2], [0, 3, 4]], 5)                                     # a bow-tie
    with pytest.raises(ValueError, match="twice"):
        build([[0, 1, 2], [2, 3, 3]], 4)
    with pytest.raises(ValueError, match="outside"):
        build([[0, 1, 2], [1, 2, 4]], 4)
    with pytest.raises(ValueError, match="outside"):
        build([[0, 1, 2], [1, -1, 3]], 4)
    with pytest.raises(ValueError, match="outside"):
        build([[0, 1, 2], [1, 2 ** 32 + 3, 2]], 4)                           # must not wrap into a valid vertex
    build([[0, 1, 2], [1, 0, 3]], 4)                                         # and the handle still works afterwards


def test_apply_checks_its_argument(dev):
    from largesteps.subdivide import Subdivision
    F, V = MESHES["triangle"]
    sub = Subdivision(torch.from_numpy(F).to(dev), V)
    with pytest.raises(ValueError):
        sub.apply(torch.zeros((V + 1, 3), device=dev))
    with pytest.raises(ValueError):
        sub.apply(torch.zeros((V, 33), device=dev))
    with pytest.raises(ValueError):
        sub.apply(torch.zeros((V, 0), device=dev))
    with pytest.raises(ValueError):
        sub.apply(torch.zeros(V, device=dev))
    with pytest.raises(TypeError):
        sub.apply(torch.zeros((V, 3), dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError):
        sub.apply(torch.zeros((V, 3)))
    with pytest.raises(TypeError):
        sub.apply(np.zeros((V, 3), np.complex64))


def test_two_runs_agree_bitwise(dev):
    from largesteps.subdivide import Subdivision
    F, V = MESHES["icosphere2"]
    tf = torch.from_numpy(F).to(dev)
    x, runs = st.values(V, 3, 5), []
    for _ in range(2):
        sub = Subdivision(tf, V, levels=2)
        X = torch.from_numpy(x).to(dev).requires_grad_()
        Y = sub.apply(X)
        g = torch.from_numpy(st.values(sub.num_vertices, 3, 6)).to(dev)
        runs.append((sub.faces, *sub.edges, Y, torch.autograd.grad(Y, X, g)[0]))
    assert all(same(a, b) for a, b in zip(*runs))


def test_a_captured_forward_and_backward_replays_bitwise(dev):
    from largesteps.subdivide import Subdivision
    F, V = MESHES["icosphere2"]
    sub = Subdivision(torch.from_numpy(F).to(dev), V, levels=2)
    X = torch.from_numpy(st.values(V, 3, 7)).to(dev).requires_grad_()
    G = torch.from_numpy(st.values(sub.num_vertices, 3, 8)).to(dev)

    def step():
        Y = sub.apply(X)
        gX, = torch.autograd.grad((Y * G).sum(), (X,))
        return Y.detach(), gX
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(eager, out):
        assert same(a, b)


def test_the_chain_from_u_to_a_rendered_loss(dev):
    """from_differential -> apply -> normals -> rasterize / interpolate / antialias -> loss: the gradient reaches u, and the stage
    through the subdivision is S^T of the statement applied to the gradient that arrives at the fine vertices, bit for bit."""
    from largesteps import render, synthetic
    from largesteps.geometry import compute_matrix
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    from largesteps.parameterize import from_differential, to_differential
    from largesteps.subdivide import Subdivision
    v, F = synthetic.icosphere(2)
    v = synthetic.perturb(v, radial=0.05, seed=1).astype(F32)
    V = v.shape[0]
    T = topology("icosphere2")
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(F).to(dev)
    M = compute_matrix(tv, tf, lambda_=5.0)
    u = to_differential(M, tv).clone().requires_grad_()
    sub = Subdivision(tf, V)
    X = from_differential(M, u, "Cholesky")
    X.retain_grad()
    Y = sub.apply(X)
    Y.retain_grad()
    fine = sub.faces
    n = compute_vertex_normals(Y, fine, compute_face_normals(Y, fine))
    view = torch.eye(4, device=dev)
    view[2, 3] = 3.0
    mvp = render.persp_proj(45, 1, 0.1, 100, device=dev) @ view
    pos = torch.matmul(torch.nn.functional.pad(Y, (0, 1), "constant", 1.0), mvp.t())[None]
    rast = render.rasterize(render.RasterizeContext(), pos, fine, (48, 48))[0]
    assert int((rast[..., 3] != 0).sum()) > 100
    col = render.interpolate((0.5 * n + 0.5).contiguous()[None], rast, fine)[0]
    img = render.antialias(col, rast, pos, fine)
    W = torch.from_numpy(np.random.default_rng(2).standard_normal(tuple(img.shape)).astype(F32)).to(dev)
    (img * W).sum().backward()
    assert u.grad is not None and torch.isfinite(u.grad).all() and float(u.grad.abs().max()) > 0.0
    assert float(Y.grad.abs().max()) > 0.0
    assert same(X.grad, st.apply_transposed(T, Y.grad.cpu().numpy(), st.LOOP))


@pytest.mark.parametrize("fn, scheme", [("loop", st.LOOP), ("upsample", st.MIDPOINT)])
def test_the_one_shots_on_numpy_return_numpy_equal_to_the_handle(dev, fn, scheme):
    from largesteps import subdivide, synthetic
    v, F = synthetic.icosphere(1)
    one_shot = getattr(subdivide, fn)
    NV, NF = one_shot(v, F, 2)
    assert isinstance(NV, np.ndarray) and isinstance(NF, np.ndarray) and NV.dtype == F32 and NF.dtype == F.dtype
    sub = subdivide.Subdivision(torch.from_numpy(F).to(dev), v.shape[0], scheme=scheme, levels=2)
    assert same(NV, sub.apply(torch.from_numpy(v).to(dev))) and same(NF, sub.faces)
    assert NV.shape == (sub.num_vertices, 3) and NF.shape == (16 * len(F), 3)
    NV1, NF1 = one_shot(v.astype(np.float64), F.astype(np.int32))            # defaults: one level; real numbers are converted
    assert NF1.dtype == np.int32 and same(NV1, st.subdivide(F, v.shape[0], v, scheme, 1)[0])
    hn = subdivide.Subdivision(F, v.shape[0], scheme=scheme)                 # a handle on numpy faces answers in numpy
    assert isinstance(hn.faces, np.ndarray) and isinstance(hn.edges[0], np.ndarray) and isinstance(hn.apply(v), np.ndarray)
    tv = torch.from_numpy(v).to(dev).requires_grad_()                        # tensors in: tensors out, differentiable
    TV, TF = one_shot(tv, torch.from_numpy(F).to(dev))
    assert TV.requires_grad and TF.device == tv.device and same(TV, NV1)


def test_the_workspace_is_not_overrun(dev):
    """ls_subdiv_topology inside a workspace of exactly ls_subdiv_workspace_bytes with a painted zone behind it, and behind every
    output: nothing past the sizes the header states is touched."""
    import ctypes
    from largesteps import _native
    F, V = MESHES["plane4"]
    T = topology("plane4")
    m, PAD = len(F), 1024
    tf = torch.from_numpy(F).to(dev)
    need = _native.workspace_bytes("ls_subdiv_workspace_bytes", (m, V))

    def padded(nbytes):
        return torch.full((nbytes + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = [4 * 3 * m, 4 * 3 * m, 8 * 3 * m, 8 * 3 * m, 4 * V, V, 8 * V, 4 * (V + 1), 4 * 3 * m, 8 * 12 * m]
    outs = [padded(s) for s in sizes]
    ws = padded(need)
    E, status = ctypes.c_int64(0), ctypes.c_int(0)
    _native.check(_native.lib().ls_subdiv_topology(_native.ptr(tf), 8, m, V, *[_native.ptr(o) for o in outs], ctypes.byref(E), ctypes.byref(status),
                                                   _native.ptr(ws), need, 0, _native.stream_of(dev)))
    torch.cuda.synchronize(dev)
    assert E.value == T.E and status.value == 0
    for t, s in zip(outs + [ws], sizes + [need]):
        assert bool((t[s:] == 0xA5).all())
    assert same(outs[9][:sizes[9]].view(torch.int64).reshape(-1, 3), T.faces)
    assert same(outs[2][:8 * T.E].view(torch.int32).reshape(-1, 2).to(torch.int64), T.edges)
