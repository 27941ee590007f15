"""
largesteps.raycast on the device (csrc/raycast.hip) against tests/ray_statement.py: for every ray the hit parameter, the face and the
weights with the same bits, on the meshes of tests/test_distance_gpu.py that stress the LBVH's pruning (a folded sheet 1e-3 apart, a thin
tube, the 70k mesh 1000 diagonals from the origin) and the face test (repeated indices, collinear corners, a single face), with rays that
stress the slab test (axis-parallel directions, origins on the surface and 1e4 boxes away, zero and non-finite directions, ranges that
are empty or cut off the nearest face). Then any-hit, the gradients bit for bit, reproducibility across runs, streams and a captured
graph, a mesh moved under a live handle, and ambient occlusion.
"""
import ctypes

import numpy as np
import pytest
import torch

import distance_grad_statement as dg
import ray_statement as rs
from test_distance_gpu import mesh
from test_raycast_cpu import grid, inside_rays
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = np.inf
BLOCK = 256
MESHES = ["ico", "folded", "tube", "degenerate", "single"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def edges(f):
    return np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)


def rays(v, f, seed):
    """fp32 (O, D, trange (n, 2) fp64 or rows of (0, inf)): about 3 BLOCK + 17 rays, so that the last workgroup is partial"""
    rng = np.random.default_rng(seed)
    f = np.asarray(f)
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    mid, span = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) or 1.0
    e = edges(f)
    O, D = [], []

    def add(o, d):
        o, d = np.broadcast_arrays(np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64))
        O.append(o.astype(F32)); D.append(d.astype(F32))
    # random origins around the box, random directions of random length
    add(mid + rng.normal(scale=0.6 * span, size=(150, 3)), rng.normal(size=(150, 3)) * rng.uniform(0.1, 10.0, (150, 1)))
    # from a point of the box at vertices and edge midpoints
    o = mid + 0.05 * (hi - lo)
    ev = e[rng.choice(e.shape[0], 100)]
    add(o, v64[rng.choice(v.shape[0], 100)] - o)
    add(o, (v64[ev[:, 0]] + v64[ev[:, 1]]) * 0.5 - o)
    # axis-parallel directions: through random points, and exactly through vertices and edge midpoints
    axis = np.eye(3)[rng.integers(0, 3, 120)] * rng.choice([-1.0, 1.0, 2.5, -0.5], (120, 1))
    ev = e[rng.choice(e.shape[0], 40)]
    through = np.concatenate([mid + rng.uniform(-0.5, 0.5, (40, 3)) * (hi - lo), v64[rng.choice(v.shape[0], 40)], (v64[ev[:, 0]] + v64[ev[:, 1]]) * 0.5])
    add(through - axis * (2.0 * span), axis)
    # origins on the surface (vertices: exactly; face points: to fp32 rounding), tmin = 0
    fp = f[rng.choice(f.shape[0], 40)]
    w = rng.dirichlet(np.ones(3), 40)
    add(np.concatenate([v64[rng.choice(v.shape[0], 60)], (w[:, :, None] * v64[fp]).sum(1)]), rng.normal(size=(100, 3)))
    # origins 1e4 boxes away, aimed at the mesh
    far = mid + rng.normal(size=(60, 3)) * 1e4 * span
    add(far, v64[rng.choice(v.shape[0], 60)] + rng.normal(scale=0.01 * span, size=(60, 3)) - far)
    # directions and origins that hit nothing
    add(mid, [[0, 0, 0], [0, -0.0, 0], [np.nan, 1, 0], [1, np.inf, 0], [-np.inf, 0, 1], [np.nan, np.nan, np.nan]])
    add([[np.nan, 0, 0], [0, np.inf, 0], mid], [[0, 0, 1], [0, 1, 0], [1e-30, 1.0, -1e-38]])
    O, D = np.concatenate(O), np.concatenate(D)
    return O, D


def with_ranges(O, D, v, f, dev):
    """the rays plus copies of 160 of them (SEL: 60 of the far rays, which cross the whole mesh, and 100 of the rays from inside) with
    ranges built from their own first hit t0: 40 that start just past it (the second-nearest face must be found), 20 empty ones, 40
    that end exactly at it, 40 of the single point [t0, t0] and 20 with a NaN"""
    t0 = rs.closest_torch(O[SEL], D[SEL], v, f, None, dev)[0].cpu().numpy()
    base = np.stack([np.zeros(O.shape[0]), np.full(O.shape[0], INF)], 1)
    parts = [np.stack([np.nextafter(t0[:40], INF), np.full(40, INF)], 1), np.stack([t0[40:60] + 1.0, t0[40:60]], 1),
             np.stack([np.zeros(40), t0[60:100]], 1), np.stack([t0[100:140], t0[100:140]], 1),
             np.stack([np.full(20, np.nan), np.full(20, INF)], 1)]
    tr = np.concatenate([base] + parts)
    return np.concatenate([O, O[SEL]]), np.concatenate([D, D[SEL]]), tr


SEL = np.concatenate([np.arange(570, 630), np.arange(150, 250)])        # rays(): the far rays are 570 .. 629, those from inside 150 .. 349


_cases = {}


def case(name, dev):
    """a mesh, its rays and the statement's answer (evaluated on the device in fp64), computed once: (v, f, O, D, trange, (t, I, W) numpy)"""
    if name not in _cases:
        v, f = mesh(name)
        f = np.asarray(f, dtype=np.int64)
        O, D = rays(v, f, seed=len(name))
        O, D, tr = with_ranges(O, D, v, f, dev)
        want = tuple(x.cpu().numpy() for x in rs.closest_torch(O, D, v, f, tr, dev, chunk=64 if f.shape[0] > 50000 else 256))
        _cases[name] = (v, f, O, D, tr, want)
    return _cases[name]


def check_against_statement(dev, name, idx=np.int64, given=None):
    """given: the tuple `case` would return, for a mesh that is not in its table (name is then only printed)"""
    from largesteps.raycast import RayMesh
    v, f, O, D, tr, want = given or case(name, dev)
    tO, tD, ttr = to(dev, O, D, tr)
    with RayMesh(*to(dev, v, f.astype(idx))) as m:
        t, I, W = m.intersect(tO, tD, ttr[:, 0], ttr[:, 1])
        occ = m.occluded(tO, tD, ttr[:, 0], ttr[:, 1])
    assert t.dtype == torch.float64 and I.dtype == torch.int64 and W.dtype == torch.float64 and W.shape == (O.shape[0], 3) and occ.dtype == torch.bool
    t, I, W, occ = (x.cpu().numpy() for x in (t, I, W, occ))
    n_t = int((t.view(np.int64) != want[0].view(np.int64)).sum())
    n_I = int((I != want[1]).sum())
    n_W = int((W.view(np.int64) != want[2].view(np.int64)).any(1).sum())
    hits = int((want[1] >= 0).sum())
    print(f"{name}: {O.shape[0]} rays, {hits} hit; {n_t} parameters, {n_I} face ids, {n_W} weight rows differ")
    assert O.shape[0] >= 3 * BLOCK + 17 and O.shape[0] % BLOCK != 0 and 0.2 * O.shape[0] < hits < O.shape[0]
    assert n_t == 0 and n_I == 0 and n_W == 0
    assert np.array_equal(occ, I >= 0)
    return v, f, O, D, tr, (t, I, W)


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("name", MESHES)
def test_intersect_is_the_statement_bitwise(dev, name, idx):
    check_against_statement(dev, name, idx)


def test_far_from_the_origin_is_the_statement_bitwise(dev):
    """the 70k mesh 1000 diagonals from the origin: the widening of the boxes is relative to the coordinates, not to the mesh"""
    check_against_statement(dev, "bunny_translated")


@pytest.mark.parametrize("name", ["ico", "degenerate", "single"])
def test_the_statement_on_the_device_is_the_numpy_statement(dev, name):
    v, f, O, D, tr, want = case(name, dev)
    t, I, W = rs.closest(O, D, v, f, tr)
    assert np.array_equal(t.view(np.int64), want[0].view(np.int64)) and np.array_equal(I, want[1])
    assert np.array_equal(W.view(np.int64), want[2].view(np.int64))
    assert np.array_equal(rs.any_hit(O, D, v, f, tr), I >= 0)
    # the second-nearest face was asked for, and found
    n = O.shape[0] - 160
    first, second = want[1][SEL[:40]], want[1][n:n + 40]
    both = (first >= 0) & (second >= 0)
    assert (want[0][n:n + 40][both] > want[0][SEL[:40]][both]).all() and (second[both] != first[both]).all()
    if name == "ico":
        assert both.sum() >= 10
    assert np.array_equal(want[1][n + 60:n + 140], want[1][SEL[60:140]])                 # tmax = t0, and [t0, t0]: the same face
    assert (want[1][n + 40:n + 60] == -1).all() and (want[1][n + 140:] == -1).all()      # empty and NaN ranges


def test_watertight_from_inside_and_ties_go_to_the_lowest_face(dev):
    from largesteps.raycast import RayMesh
    v, f = mesh("ico")
    O, D = inside_rays(v, np.asarray(f))
    with RayMesh(*to(dev, v, f)) as m:
        t, I, W = m.intersect(*to(dev, O, D))
        assert bool((I >= 0).all()) and bool(m.occluded(*to(dev, O, D)).all())
    want = rs.closest(O, D, v, f)
    assert np.array_equal(t.cpu().numpy().view(np.int64), want[0].view(np.int64)) and np.array_equal(I.cpu().numpy(), want[1])


def test_numpy_input_empty_queries_and_null_outputs(dev):
    from largesteps import _native
    from largesteps.raycast import RayMesh, ray_mesh_intersect
    v, f, O, D, tr, want = case("ico", dev)
    t, I, W = ray_mesh_intersect(O.astype(np.float64), D, v.astype(np.float64), f.astype(np.int32), tr[:, 0], tr[:, 1])
    assert isinstance(t, np.ndarray) and t.dtype == np.float64 and I.dtype == np.int64 and W.shape == (O.shape[0], 3)
    assert np.array_equal(t.view(np.int64), want[0].view(np.int64)) and np.array_equal(I, want[1]) and np.array_equal(W.view(np.int64), want[2].view(np.int64))
    n = O.shape[0] - 160
    t, I, W = ray_mesh_intersect(O[:n], D[:n], v, f)                   # the default range: no trange array at all
    assert np.array_equal(t.view(np.int64), want[0][:n].view(np.int64)) and np.array_equal(I, want[1][:n])
    t, I, W = ray_mesh_intersect(O[:n], D[:n], v, f, tmin=0.25, tmax=np.full(n, 2.0))
    w2 = rs.closest(O[:n], D[:n], v, f, np.stack([np.full(n, 0.25), np.full(n, 2.0)], 1))
    assert np.array_equal(t.view(np.int64), w2[0].view(np.int64)) and np.array_equal(I, w2[1])
    t, I, W = ray_mesh_intersect(np.zeros((0, 3)), np.zeros((0, 3)), v, f)
    assert t.shape == (0,) and I.shape == (0,) and W.shape == (0, 3)
    tO, tD = to(dev, O, D)
    with RayMesh(*to(dev, v, f)) as m:
        t, I, W = m.intersect(tO[:0], tD[:0])
        assert t.shape == (0,) and t.device == dev and m.occluded(tO[:0], tD[:0]).shape == (0,)
        occ = m.occluded(O, D, tr[:, 0], tr[:, 1])
        assert isinstance(occ, np.ndarray) and occ.dtype == np.bool_ and np.array_equal(occ, want[1] >= 0)
        # every output NULL, and one at a time
        lib, st = _native.lib(), _native.stream_of(dev)
        ttr, = to(dev, tr)
        args = (m._h, _native.ptr(tO), _native.ptr(tD), O.shape[0], _native.ptr(ttr))
        assert lib.ls_mesh_ray_closest(*args, None, None, None, st) == 0
        only_t = torch.empty(O.shape[0], dtype=torch.float64, device=dev)
        only_I = torch.empty(O.shape[0], dtype=torch.int64, device=dev)
        assert lib.ls_mesh_ray_closest(*args, _native.ptr(only_t), None, None, st) == 0
        assert lib.ls_mesh_ray_closest(*args, None, _native.ptr(only_I), None, st) == 0
        assert np.array_equal(only_t.cpu().numpy().view(np.int64), want[0].view(np.int64)) and np.array_equal(only_I.cpu().numpy(), want[1])
        # the distance queries of the same handle still answer
        d2, _, _ = m.squared_distance(tO[:64])
        assert d2.shape == (64,)
    with pytest.raises(TypeError):
        ray_mesh_intersect(O, tD, v, f)                                # numpy and tensors mixed
    with pytest.raises(TypeError):
        ray_mesh_intersect(tO.double(), tD, *to(dev, v, f))


# ---- the gradient ------------------------------------------------------------------------------------------------------------------
def run(dev, v, f, O, D, g, tr=None, idx=np.int64, need=(True, True, True), handle=None):
    """forward and backward through the public interface: (t, I, W, gO, gD, gV) tensors"""
    from largesteps.raycast import RayMesh
    tO, tD = (x.requires_grad_(r) for x, r in zip(to(dev, O, D), need[:2]))
    V = to(dev, v)[0].requires_grad_(need[2])
    m = handle if handle is not None else RayMesh(V, to(dev, np.asarray(f).astype(idx))[0])
    try:
        if handle is not None:
            m.update(V)
        rng = () if tr is None else to(dev, tr[:, 0], tr[:, 1])
        t, I, W = m.intersect(tO, tD, *rng)
        assert t.requires_grad and t.dtype == torch.float64 and not I.requires_grad and not W.requires_grad
        # a miss has t = inf: its incoming gradient is taken as 0 so that the loss is finite (its terms are zero either way)
        (torch.where(I >= 0, t, torch.zeros_like(t)) * to(dev, g)[0]).sum().backward()
    finally:
        if handle is None:
            m.close()
    return t.detach(), I, W, tO.grad, tD.grad, V.grad


def check_gradients(dev, name, v, f, O, D, tr, idx=np.int64):
    from largesteps.raycast import RayMesh
    g = np.random.default_rng(len(name)).uniform(-1.0, 2.0, O.shape[0])
    t, I, W, gO, gD, gV = run(dev, v, f, O, D, g, tr, idx)
    with RayMesh(*to(dev, v, f)) as m:
        vptr, order = (x.cpu().numpy() for x in m._corner_ranks())
    t, I, W = (x.cpu().numpy() for x in (t, I, W))
    gin = np.where(I >= 0, g, 0.0)
    tO, tD, tV = rs.terms(O, D, v, f, I, W, t, gin)
    assert gO.dtype == torch.float32 and gO.shape == O.shape and gD.shape == D.shape and gV.shape == v.shape
    gO, gD, gV = (x.cpu().numpy() for x in (gO, gD, gV))
    n_O = int((gO.view(np.int32) != tO.astype(F32).view(np.int32)).any(1).sum())
    n_D = int((gD.view(np.int32) != tD.astype(F32).view(np.int32)).any(1).sum())
    want = dg.vertex_sums(dg.face_rows(tV.astype(F32).reshape(-1, 9), dg.keys(I, f.shape[0]), f.shape[0]), vptr, order)
    n_V = int((gV.view(np.int32) != want.view(np.int32)).any(1).sum())
    per_face = np.bincount(I[I >= 0], minlength=f.shape[0])
    print(f"{name}: {O.shape[0]} rays, {int((I >= 0).sum())} hit, most on a face {int(per_face.max())}, faces without a ray {int((per_face == 0).sum())}; "
          f"{n_O} gO rows, {n_D} gD rows, {n_V} gV rows differ")
    assert n_O == 0 and n_D == 0 and n_V == 0
    assert not gO[I < 0].any() and not gD[I < 0].any()
    return per_face


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("name", MESHES)
def test_gradients_are_the_statement_bitwise(dev, name, idx):
    """gO and gD are the rounded terms, gV the ordered fp32 sums; `single` puts every hit on one face: the wave-strided path of seg_sum"""
    v, f, O, D, tr, _ = case(name, dev)
    per_face = check_gradients(dev, name, v, f, O, D, tr, idx)
    if name == "single":
        assert per_face.max() > 64
    if name == "ico":
        assert (per_face == 0).any()


def test_gradients_past_one_sort_workgroup_and_one_key_byte(dev):
    """2562 rays from inside the 1280-face icosphere: three sort workgroups of 1024, two byte passes; then 25 rays: most faces get none"""
    v, f = mesh("ico")
    f = np.asarray(f, dtype=np.int64)
    O, D = inside_rays(v, f)
    assert O.shape[0] > 2 * 1024 and f.shape[0] > 256
    check_gradients(dev, "inside", v, f, O, D, None)
    per_face = check_gradients(dev, "few", v, f, O[:25], D[:25], None)
    assert (per_face == 0).sum() > 1200
    from largesteps.raycast import RayMesh
    V = to(dev, v)[0].requires_grad_()
    with RayMesh(V, to(dev, f)[0]) as m:                                # no rays at all: a zero gradient
        t, _, _ = m.intersect(torch.zeros((0, 3), device=dev).requires_grad_(), torch.zeros((0, 3), device=dev))
        t.sum().backward()
    assert V.grad.shape == v.shape and not bool(V.grad.any())


def test_only_one_input_requires_grad_and_nothing_requires_grad(dev):
    from largesteps.raycast import RayMesh, ray_mesh_intersect
    v, f, O, D, tr, want = case("folded", dev)
    g = np.random.default_rng(1).uniform(-1.0, 2.0, O.shape[0])
    both = run(dev, v, f, O, D, g, tr)
    for k in range(3):
        need = tuple(j == k for j in range(3))
        one = run(dev, v, f, O, D, g, tr, need=need)
        for j in range(3):
            assert (one[3 + j] is None) == (j != k)
        assert torch.equal(bits(one[3 + k]), bits(both[3 + k]))
    tO, tD, tt0, tt1, V, tf = to(dev, O, D, tr[:, 0], tr[:, 1], v, f)
    with RayMesh(V, tf) as m:
        plain = m.intersect(tO, tD, tt0, tt1)
        with torch.no_grad(), RayMesh(V.clone().requires_grad_(), tf) as mg:
            quiet = mg.intersect(tO.clone().requires_grad_(), tD, tt0, tt1)
    for out in (plain, quiet, ray_mesh_intersect(tO, tD, V, tf, tt0, tt1)):
        assert out[0].requires_grad is False and out[0].grad_fn is None
        for a, b in zip(out, want):
            assert np.array_equal(a.cpu().numpy().view(np.int64), b.view(np.int64))
    for a, b in zip(ray_mesh_intersect(tO.clone().requires_grad_(), tD, V, tf, tt0, tt1), want):      # the differentiable path: the same bits
        assert np.array_equal(a.detach().cpu().numpy().view(np.int64), b.view(np.int64))


def test_two_runs_and_another_stream_give_identical_bits(dev):
    v, f, O, D, tr, _ = case("single", dev)
    v2, f2, O2, D2, tr2, _ = case("ico", dev)
    g, g2 = np.linspace(-1.0, 2.0, O.shape[0]), np.linspace(2.0, -1.0, O2.shape[0])
    first = [run(dev, v, f, O, D, g, tr), run(dev, v2, f2, O2, D2, g2, tr2)]
    again = [run(dev, v, f, O, D, g, tr), run(dev, v2, f2, O2, D2, g2, tr2)]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        other = [run(dev, v, f, O, D, g, tr), run(dev, v2, f2, O2, D2, g2, tr2)]
    torch.cuda.current_stream(dev).wait_stream(s)
    for a, b, c in zip(first, again, other):
        for x, y, z in zip(a, b, c):
            assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))


def test_a_captured_forward_and_backward_replays_bitwise(dev):
    from largesteps.raycast import RayMesh
    v, f, O, D, tr, _ = case("ico", dev)
    V, tO, tD = (x.requires_grad_() for x in to(dev, v, O, D))
    G, t0, t1 = to(dev, np.linspace(-1.0, 2.0, O.shape[0]), tr[:, 0], tr[:, 1])
    with RayMesh(V, to(dev, f)[0]) as m:
        def step():
            t, I, W = m.intersect(tO, tD, t0, t1)
            gO, gD, gV = torch.autograd.grad((torch.where(I >= 0, t, torch.zeros_like(t)) * G).sum(), (tO, tD, V))
            return t.detach(), I, W, gO, gD, gV, m.occluded(tO, tD, t0, t1)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            eager = [x.clone() for x in step()]                  # the warm-up: builds the corner ranking
        torch.cuda.current_stream(dev).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        for a, b in zip(eager, out):
            assert torch.equal(bits(a), bits(b))
        assert bool(eager[1].ge(0).any()) and bool(eager[5].any())


def test_update_answers_like_a_fresh_handle_and_fences_the_backward(dev):
    from largesteps.raycast import RayMesh
    v, f, O, D, tr, _ = case("ico", dev)
    v2 = (synthetic.perturb(v, radial=0.08, seed=9).astype(F32) + F32(0.25)).astype(F32)
    tf, tO, tD = to(dev, f, O, D)
    tO.requires_grad_()
    V1, V2 = to(dev, v)[0].requires_grad_(), to(dev, v2)[0].requires_grad_()
    with RayMesh(V1, tf) as m, RayMesh(V2, tf) as fresh:
        stale = m.intersect(tO, tD)[0]
        m.update(V2)
        for a, b in zip(m.intersect(tO, tD), fresh.intersect(tO, tD)):
            assert torch.equal(bits(a.detach()), bits(b.detach()))
        assert torch.equal(m.occluded(tO, tD), fresh.occluded(tO, tD))
        want = rs.closest_torch(O, D, v2, f, None, dev)
        assert torch.equal(bits(m.intersect(tO, tD)[0].detach()), bits(want[0])) and torch.equal(m.intersect(tO, tD)[1], want[1])
        with pytest.raises(RuntimeError, match="updated"):
            torch.nan_to_num(stale, posinf=0.0).sum().backward()

        def loss(h):
            t, I, _ = h.intersect(tO, tD)
            return torch.where(I >= 0, t, torch.zeros_like(t)).sum()
        ga, = torch.autograd.grad(loss(m), V2)
        gb, = torch.autograd.grad(loss(fresh), V2)
        assert torch.equal(bits(ga), bits(gb)) and bool(ga.any())
        with torch.no_grad():
            V2.mul_(1.5)
        with pytest.raises(RuntimeError, match="in place"):
            m.intersect(tO, tD)
        m.update(V2)
        loss(m).backward()


def test_the_workspace_is_checked(dev):
    from largesteps import _native
    from largesteps.raycast import RayMesh
    v, f, O, D, tr, want = case("ico", dev)
    n = O.shape[0]
    tO, tD, tt, tI, tW, G = to(dev, O, D, want[0], want[1], want[2], np.ones(n))
    with RayMesh(*to(dev, v, f)) as m:
        vptr, order = m._corner_ranks()
        gV = torch.empty((v.shape[0], 3), dtype=torch.float32, device=dev)
        need = ctypes.c_size_t(0)
        _native.check(_native.lib().ls_mesh_ray_backward_workspace_bytes(n, f.shape[0], ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        args = (m._h, _native.ptr(tO), _native.ptr(tD), n, _native.ptr(tI), _native.ptr(tW), _native.ptr(tt), _native.ptr(G), _native.ptr(vptr),
                _native.ptr(order), None, None, _native.ptr(gV), _native.ptr(ws))
        assert _native.lib().ls_mesh_ray_backward(*args, need.value - 1, _native.stream_of(dev)) == _native.LS_E_WORKSPACE
        assert _native.lib().ls_mesh_ray_backward(*args, need.value, _native.stream_of(dev)) == 0
        torch.cuda.synchronize(dev)


# ---- ambient occlusion -------------------------------------------------------------------------------------------------------------
def test_ambient_occlusion_inside_a_closed_mesh_and_above_an_open_plane(dev):
    from largesteps.raycast import ambient_occlusion
    v, f = synthetic.icosphere(8)
    v = v.astype(F32)
    f = np.asarray(f, dtype=np.int64)
    # the face centroids of a closed sphere with normals pointing in: every ray ends on the sphere
    c = v.astype(np.float64)[f].mean(1)
    nrm = -c / np.linalg.norm(c, axis=1, keepdims=True)
    ao = ambient_occlusion(*to(dev, v, f, c.astype(F32), nrm.astype(F32)), 64, seed=3)
    assert ao.dtype == torch.float32 and ao.shape == (f.shape[0],) and ao.device == dev
    assert bool((ao == 1.0).all())
    # points on an open flat sheet with normals pointing away from it: nothing above
    pv, pf = grid(24, 1.0 / 32)
    p = pv.astype(np.float64)[pf].mean(1)[:300]
    ao = ambient_occlusion(pv, pf, p, np.broadcast_to([0.0, 0.0, 1.0], p.shape), 64)
    assert isinstance(ao, np.ndarray) and ao.dtype == np.float32 and ao.shape == (300,) and not ao.any()
    # in the valleys of the sine sheet the crests hide a part of the sky: the same seed gives the same values, another seed others
    sv, sf = synthetic.plane(24)
    q = sv.astype(np.float64)[np.asarray(sf)].mean(1)[::5]
    up = np.broadcast_to([0.0, 0.0, 1.0], q.shape)
    a1 = ambient_occlusion(sv, sf, q, up, 32, seed=5)
    a2 = ambient_occlusion(sv, sf, q, up, 32, seed=5)
    a3 = ambient_occlusion(sv, sf, q, up, 32, seed=6)
    assert np.array_equal(a1, a2) and ((a1 >= 0) & (a1 <= 1)).all() and (a1 > 0).any() and (a1 < 1).any()
    assert not np.array_equal(a1, a3)
