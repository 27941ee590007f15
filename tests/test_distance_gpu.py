"""
largesteps.distance on the device (csrc/distance.hip) against tests/distance_statement.py evaluated on the device in fp64: for every
query point the squared distance and the closest point with the same bits and the same face id, on meshes that stress the LBVH's
pruning (folded sheets 1e-3 apart, a thin tube, the 70k mesh 1000 diagonals from the origin, points far outside the box) and the
leaf test (repeated indices, collinear corners, a single face, points on vertices and edges where several faces tie). Then libigl's
hausdorff: the statement's value, symmetric, reproducible, through a kept MeshDistance, on another stream, in the figure's call form,
and at 1M vertices on a sample.
"""
import numpy as np
import pytest
import torch

import distance_statement as ds
from test_remesh_cpu import torus
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def tube(m=600, k=12, radius=1e-3):
    """an open tube of length 1 and radius 1e-3 along x: m rings of k vertices"""
    x = np.arange(m) / (m - 1)
    w = np.arange(k) * 2 * np.pi / k
    X, W = np.meshgrid(x, w, indexing="ij")
    v = np.stack([X, radius * np.cos(W), radius * np.sin(W)], -1).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(m - 1), np.arange(k), indexing="ij")
    a, b, c, d = i * k + j, (i + 1) * k + j, (i + 1) * k + (j + 1) % k, i * k + (j + 1) % k
    return v, np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])


def with_degenerate_faces(v, f):
    """the mesh plus faces that repeat an index or have exactly collinear corners (on a grid of binary fractions)"""
    n = v.shape[0]
    line = np.array([[0.5, 0.5, 0.5], [0.75, 0.625, 0.5], [1.0, 0.75, 0.5], [0.0, 0.25, 0.5]], dtype=F32)
    extra = np.array([[0, 0, 1], [2, 3, 3], [4, 4, 4], [n, n + 1, n + 2], [n + 2, n + 3, n], [n + 1, n + 1, n + 3], [5, 5, 6]])
    return np.concatenate([v, line]), np.concatenate([f, extra])


def mesh(name):
    if name == "ico":
        v, f = synthetic.icosphere(8)
        return synthetic.perturb(v, radial=0.05, seed=2).astype(F32), f
    if name == "plane":
        return synthetic.plane(24)
    if name == "torus":
        return torus()
    if name == "folded":
        return synthetic.folded_sheet(60)
    if name == "tube":
        return tube()
    if name == "degenerate":
        v, f = synthetic.icosphere(6)
        return with_degenerate_faces(v, f)
    if name == "single":
        return np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.2], [0.3, 0.9, -0.4]], dtype=F32), np.array([[0, 1, 2]])
    if name == "bunny_translated":
        v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
        v64 = v.astype(np.float64)
        diag = float(np.linalg.norm(v64.max(0) - v64.min(0)))
        return (v64 + 1000.0 * diag).astype(F32), f
    raise KeyError(name)


def probes(v, f, n, seed):
    """fp32 query points: vertices (every face around them ties at 0), points on edges, points near the surface, far from it (3 and
    1e4 boxes) and on the far side of the origin"""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    span = float(np.linalg.norm(hi - lo)) or 1.0
    on_v = v64[rng.choice(v.shape[0], n)]
    e = f[rng.choice(f.shape[0], n)]
    k = rng.integers(0, 3, n)
    t = rng.uniform(0.0, 1.0, (n, 1))
    a, b = v64[e[np.arange(n), k]], v64[e[np.arange(n), (k + 1) % 3]]
    on_e = np.concatenate([(a + b) * 0.5, a + t * (b - a)])
    near = v64[rng.choice(v.shape[0], n)] + rng.normal(scale=0.02 * span, size=(n, 3))
    far = (lo + hi) / 2 + rng.normal(scale=3.0 * span, size=(n, 3))
    very_far = rng.normal(scale=1e4 * span, size=(n // 4 + 1, 3))
    return np.concatenate([on_v, on_e, near, far, very_far, -v64[:n]]).astype(F32)


def check_against_statement(dev, v, f, p, idx=np.int64, pchunk=512, tchunk=16384):
    from largesteps.distance import MeshDistance
    P = torch.from_numpy(p).to(dev)
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(f).astype(idx)).to(dev)) as m:
        d2, I, C = m.squared_distance(P)
        mx = m.max_squared_distance(P)
    want_d2, want_I, want_C = ds.squared_distance_torch(P, v, f, dev, pchunk=pchunk, tchunk=tchunk)
    assert d2.dtype == torch.float64 and I.dtype == torch.int64 and C.dtype == torch.float64 and C.shape == (p.shape[0], 3)
    assert bool(torch.isfinite(d2).all()) and bool(torch.isfinite(C).all())
    n_d2 = int((d2.view(torch.int64) != want_d2.view(torch.int64)).sum())
    n_I = int((I != want_I).sum())
    n_C = int((C.view(torch.int64) != want_C.view(torch.int64)).any(1).sum())
    assert n_d2 == 0 and n_I == 0 and n_C == 0, f"of {p.shape[0]} points: {n_d2} squared distances, {n_I} face ids, {n_C} closest points differ"
    assert mx.shape == () and torch.equal(mx, want_d2.max())
    return d2, I, C


SMALL = ["ico", "plane", "torus", "folded", "tube", "degenerate", "single"]


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("name", SMALL)
def test_query_is_the_statement_bitwise(dev, name, idx):
    v, f = mesh(name)
    check_against_statement(dev, v, f, probes(v, f, 512, seed=len(name)), idx)


def test_query_far_from_the_origin_is_the_statement_bitwise(dev):
    """the 70k mesh 1000 diagonals from the origin: fp32 box distances would round above the truth there; the fp64 bound does not"""
    v, f = mesh("bunny_translated")
    check_against_statement(dev, v, f, probes(v, f, 768, seed=7), pchunk=256, tchunk=65536)


def test_ties_on_vertices_go_to_the_lowest_face(dev):
    v, f = mesh("ico")
    d2, I, C = check_against_statement(dev, v, f, v)
    assert not bool(d2.any())
    lowest = np.full(v.shape[0], f.shape[0])
    np.minimum.at(lowest, f.reshape(-1), np.repeat(np.arange(f.shape[0]), 3))
    assert np.array_equal(I.cpu().numpy(), lowest)
    assert torch.equal(C, torch.from_numpy(v).to(dev).double())


def test_numpy_input_and_empty_queries(dev):
    from largesteps.distance import MeshDistance, point_mesh_squared_distance
    v, f = mesh("torus")
    p = probes(v, f, 64, seed=1)
    d2, I, C = point_mesh_squared_distance(p.astype(np.float64), v.astype(np.float64), f.astype(np.int32))
    assert isinstance(d2, np.ndarray) and d2.dtype == np.float64 and I.dtype == np.int64 and C.shape == (p.shape[0], 3)
    want = ds.squared_distance(p, v, f)
    assert np.array_equal(d2, want[0]) and np.array_equal(I, want[1]) and np.array_equal(C, want[2])
    d2, I, C = point_mesh_squared_distance(np.zeros((0, 3)), v, f)
    assert d2.shape == (0,) and I.shape == (0,) and C.shape == (0, 3)
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) as m:
        d2, I, C = m.squared_distance(torch.zeros((0, 3), device=dev))
        assert d2.shape == (0,) and d2.device == dev
        assert float(m.max_squared_distance(torch.zeros((0, 3), device=dev))) == 0.0
        assert m.max_squared_distance(p) == float(want[0].max())


def test_argument_errors(dev):
    from largesteps.distance import MeshDistance, hausdorff
    v, f = mesh("torus")
    with pytest.raises(IndexError):
        MeshDistance(v, np.concatenate([f, [[0, 1, v.shape[0]]]]))
    with pytest.raises(IndexError):
        MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(np.concatenate([f, [[0, -1, 2]]]).astype(np.int32)).to(dev))
    with pytest.raises(TypeError):
        MeshDistance(torch.from_numpy(v).to(dev).double(), torch.from_numpy(f).to(dev))
    with pytest.raises(ValueError):
        hausdorff(v, f, v, np.zeros((0, 3), np.int64))


def pair():
    va, fa = synthetic.icosphere(10)
    va = synthetic.perturb(va, radial=0.03, seed=11).astype(F32)
    vb, fb = synthetic.icosphere(7)
    return va, fa, synthetic.perturb(vb, radial=0.05, seed=12).astype(F32), fb


def test_hausdorff_is_the_statement_and_symmetric(dev):
    from largesteps.distance import MeshDistance, hausdorff
    va, fa, vb, fb = pair()
    want = ds.hausdorff(va, fa, vb, fb, squared=ds.squared_on(dev, pchunk=512, tchunk=8192))
    got = hausdorff(va, fa, vb, fb)
    assert isinstance(got, float) and got == want and got > 0.0
    assert hausdorff(vb, fb, va, fa) == got
    ta, tfa, tb, tfb = (torch.from_numpy(x).to(dev) for x in (va, fa.astype(np.int32), vb, fb))
    assert hausdorff(ta, tfa, tb, tfb) == got
    with MeshDistance(vb, fb) as m:
        assert m.hausdorff(va, fa) == got
        assert m.hausdorff(ta, tfa) == got


def test_two_calls_give_identical_bits(dev):
    from largesteps.distance import MeshDistance, hausdorff
    v, f = mesh("folded")
    p = torch.from_numpy(probes(v, f, 2048, seed=4)).to(dev)
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) as m:
        r1 = m.squared_distance(p)
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) as m:
        r2 = m.squared_distance(p)
        r3 = m.squared_distance(p)
    for a, b, c in zip(r1, r2, r3):
        assert torch.equal(a.view(torch.int64) if a.is_floating_point() else a, b.view(torch.int64) if b.is_floating_point() else b)
        assert torch.equal(b, c)
    va, fa, vb, fb = pair()
    assert hausdorff(va, fa, vb, fb) == hausdorff(va, fa, vb, fb)


def test_a_non_default_stream(dev):
    from largesteps.distance import MeshDistance, hausdorff
    v, f = mesh("ico")
    p = torch.from_numpy(probes(v, f, 1024, seed=9)).to(dev)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    with MeshDistance(tv, tf) as m:
        want = m.squared_distance(p)
        want_max = m.max_squared_distance(p).item()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with MeshDistance(tv, tf) as m:
            got = m.squared_distance(p)
            got_max = m.max_squared_distance(p)
        va, fa, vb, fb = pair()
        h = hausdorff(va, fa, vb, fb)
    torch.cuda.current_stream(dev).wait_stream(s)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert got_max.item() == want_max
    assert h == hausdorff(va, fa, vb, fb)


def test_the_figure_block_on_a_recorded_trajectory(dev):
    """figures/comparison/generate_data.py: d = hausdorff(verts[it], fa, vb, fb) + hausdorff(vb, fb, verts[it], fa) on every 10th
    recorded step, with numpy float64 vertices and the int faces the figure passes"""
    from largesteps.distance import hausdorff
    va, fa = synthetic.icosphere(12)
    vb, fb = synthetic.icosphere(9)
    vb = synthetic.perturb(vb, radial=0.05, seed=3).astype(np.float64)
    start = synthetic.perturb(va, radial=0.2, seed=4).astype(np.float64)
    target = va.astype(np.float64)
    verts = [start + (target - start) * (s / 40.0) for s in range(41)]
    fa = fa.astype(np.int64)
    its = list(range(0, len(verts), 10))
    d_hausdorff = np.zeros(len(its))
    for k, it in enumerate(its):
        d_hausdorff[k] = hausdorff(verts[it], fa, vb, fb) + hausdorff(vb, fb, verts[it], fa)
    squared = ds.squared_on(dev, pchunk=512, tchunk=8192)
    want = np.array([2 * ds.hausdorff(verts[it], fa, vb, fb, squared=squared) for it in its])
    assert np.array_equal(d_hausdorff, want)
    assert d_hausdorff[0] > d_hausdorff[-1] > 0.0


def test_one_million_vertices_on_a_sample(dev):
    """a 1M-vertex sphere against its perturbed copy: every point queried on the device, a random 20k of them (and the 1024 farthest)
    checked against the brute force over all 2M faces"""
    from largesteps.distance import MeshDistance, hausdorff
    vb, fb, _ = synthetic.config_mesh("cfg4b_sphere1m")
    va = synthetic.perturb(vb, radial=0.01, seed=21).astype(F32)
    P = torch.from_numpy(va).to(dev)
    with MeshDistance(torch.from_numpy(vb).to(dev), torch.from_numpy(fb).to(dev)) as m:
        d2, I, C = m.squared_distance(P)
        mx = m.max_squared_distance(P)
    assert torch.equal(mx, d2.max())
    rng = np.random.default_rng(0)
    far = torch.argsort(d2, descending=True, stable=True)[:1024].cpu().numpy()
    idx = np.union1d(rng.choice(va.shape[0], 20000, replace=False), far)
    sel = torch.from_numpy(idx).to(dev)
    want_d2, want_I, want_C = ds.squared_distance_torch(P[sel], vb, fb, dev, pchunk=256, tchunk=65536)
    assert torch.equal(d2[sel].view(torch.int64), want_d2.view(torch.int64))
    assert torch.equal(I[sel], want_I)
    assert torch.equal(C[sel].view(torch.int64), want_C.view(torch.int64))
    h = hausdorff(va, fb, vb, fb)
    assert h == hausdorff(vb, fb, va, fb) and h * h >= float(mx) * (1 - 1e-15)
