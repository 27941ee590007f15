"""
The remesher's contract on the CPU: tests/remesh_statement.py (the numpy statement of csrc/remesh.hip, phase for phase) keeps a
mesh edge-manifold, oriented, of the same Euler characteristic and with its boundary untouched; lattices at their own edge length
are fixed points; bad input raises ValueError; five iterations reach a measured quality.
"""
import os

import numpy as np
import pytest

import remesh_statement as rs
from largesteps import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def torus(n=24, m=12, R=1.0, r=0.35):
    u, w = np.arange(n) * 2 * np.pi / n, np.arange(m) * 2 * np.pi / m
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, f


def lattice(n=9, s=1.0):
    """equilateral triangle lattice patch (n x n vertices, rows shifted by half an edge), edge length s, consistently oriented"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([(x + 0.5 * (y % 2)) * s, y * s * np.sqrt(3.0) / 2, 0 * x], -1).reshape(-1, 3).astype(F32)
    f = []
    for r in range(n - 1):
        for c in range(n - 1):
            i, j = r * n + c, (r + 1) * n + c
            if r % 2 == 0:
                f += [(i, i + 1, j), (i + 1, j + 1, j)]
            else:
                f += [(i, j + 1, j), (i, i + 1, j + 1)]
    return v, np.array(f, dtype=np.int64)


def golden_meshes():
    out = {}
    for fn in ("reference_golden.npz", "reference_meshgeom.npz"):
        z = np.load(os.path.join(HERE, "golden", fn))
        for k in z.files:
            if k.endswith("/faces"):
                name = k[:-len("/faces")]
                v, f = z[name + "/verts"].astype(F32), z[k].astype(np.int64)
                try:
                    rs.validate(v, f)
                except ValueError:
                    continue
                if np.unique(v, axis=0).shape[0] == v.shape[0] and f.shape[0] >= 4:
                    out[f"{fn.split('_')[1].split('.')[0]}:{name}"] = (v, f)
    return out


def meshes():
    ico = synthetic.icosphere(6)
    m = {
        "icosphere": (ico[0].astype(F32), ico[1]),
        "icosphere_perturbed": (synthetic.perturb(ico[0], radial=0.05, seed=3).astype(F32), ico[1]),
        "torus": torus(),
        "plane": tuple(x for x in synthetic.plane(10)),
    }
    m.update(golden_meshes())
    return m


MESHES = meshes()


def avg_edge(v, f):
    return float(np.linalg.norm(v[f[:, [1, 2, 0]]].astype(np.float64) - v[f], axis=2).mean())


def edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def boundary_verts(f):
    t = rs.Topo(np.zeros((int(f.max()) + 1, 3), F32), f)
    return np.unique(t.org[t.twin < 0])


def check_invariants(v0, f0, v, f):
    rs.validate(v, f)                                    # edge-manifold, oriented, one fan per vertex
    assert v.dtype == F32 and np.isfinite(v).all()
    chi0 = v0.shape[0] - edges(f0).shape[0] + f0.shape[0]
    assert v.shape[0] - edges(f).shape[0] + f.shape[0] == chi0, "Euler characteristic changed"
    assert np.unique(np.sort(f, axis=1), axis=0).shape[0] == f.shape[0], "duplicate face"
    assert np.bincount(f.reshape(-1), minlength=v.shape[0]).min() > 0, "unreferenced vertex"
    n = rs.tri_normal(v[f[:, 0]].astype(np.float64), v[f[:, 1]].astype(np.float64), v[f[:, 2]].astype(np.float64))
    assert (np.linalg.norm(n, axis=1) > 0).all(), "degenerate face"
    # the boundary: the same positions, bit for bit, and the same boundary loop sizes
    b0, b = boundary_verts(f0), boundary_verts(f)
    assert b.size == b0.size
    assert np.array_equal(np.unique(v0[b0].view(np.uint32), axis=0), np.unique(v[b].view(np.uint32), axis=0))


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("scale", [0.5, 1.0, 2.0])
def test_full_iterations_keep_invariants(name, scale):
    v0, f0 = MESHES[name]
    h = F32(scale * avg_edge(v0, f0))
    v, f = rs.remesh_botsch(v0, f0, 2, h, True)
    check_invariants(v0, f0, v, f)


@pytest.mark.parametrize("name", ["icosphere_perturbed", "plane"])
def test_each_phase_keeps_invariants(name):
    v, f = MESHES[name]
    h = F32(0.5 * avg_edge(v, f))
    V0, F0 = v, f
    for fn in (rs.split_round, rs.collapse_round, rs.flip_round):
        v2, f2, n = fn(v, f, h)
        check_invariants(V0, F0, v2, f2)
        v, f = v2, f2
    v2, f2, _ = rs.relax(v, f)
    check_invariants(V0, F0, v2, f2)
    v2, f2, _ = rs.project(v2, f2, V0, F0)
    check_invariants(V0, F0, v2, f2)


def test_lattice_is_a_fixed_point():
    v, f = lattice(9, 1.0)
    rs.validate(v, f)
    h = F32(1.0)
    assert rs.split_round(v, f, h)[2] == 0
    assert rs.collapse_round(v, f, h)[2] == 0
    v2, f2, n = rs.flip_round(v, f, h)
    assert np.array_equal(v2, v)
    bnd = np.zeros(v.shape[0], dtype=bool)
    bnd[boundary_verts(f)] = True
    e0, e1 = {tuple(e) for e in edges(f)}, {tuple(e) for e in edges(f2)}
    t = rs.Topo(v, f)
    for e in e0 ^ e1:                                    # every changed edge touches the boundary through an end or an opposite vertex
        if e in e0:
            h_ = np.nonzero(((t.org == e[0]) & (t.dst == e[1])) | ((t.org == e[1]) & (t.dst == e[0])))[0]
            touch = set(e) | {int(f.reshape(-1)[3 * (x // 3) + (x + 2) % 3]) for x in h_}
        else:
            touch = set(e)
            t2 = rs.Topo(v2, f2)
            h_ = np.nonzero(((t2.org == e[0]) & (t2.dst == e[1])) | ((t2.org == e[1]) & (t2.dst == e[0])))[0]
            touch |= {int(f2.reshape(-1)[3 * (x // 3) + (x + 2) % 3]) for x in h_}
        assert bnd[list(touch)].any(), f"interior flip of {e}"
    # no interior vertex of the lattice changed valence-6 status
    inner = ~bnd
    assert (rs.Topo(v2, f2).val[inner] == 6).all()


def test_invalid_input_raises():
    v, f = synthetic.icosphere(3)
    v = v.astype(F32)
    with pytest.raises(ValueError):                     # a face repeats a vertex
        rs.validate(v, np.concatenate([f, [[0, 0, 1]]]))
    g = f.copy()
    g[0] = g[0, ::-1]
    with pytest.raises(ValueError):                     # one face turned over
        rs.validate(v, g)
    with pytest.raises(ValueError):                     # three faces on one edge
        rs.validate(np.concatenate([v, [[5, 5, 5]]]).astype(F32), np.concatenate([f, [[f[0, 0], f[0, 1], v.shape[0]]]]))
    bow = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], F32)
    with pytest.raises(ValueError):                     # bow tie: two fans at vertex 0
        rs.validate(bow, np.array([[0, 1, 2], [0, 3, 4]]))


# Quality after 5 iterations at h = 0.5 * average edge length, measured with the statement (floors a little below):
#   perturbed icosphere(6)  edges in [lo, hi]: 0.9935   valence-6 vertices: 0.9535
#   torus 24 x 12           edges in [lo, hi]: 0.9612   valence-6 vertices: 0.7693
@pytest.mark.parametrize("name,edge_floor,val6_floor", [("icosphere_q", 0.99, 0.95), ("torus", 0.96, 0.76)])
def test_quality_after_five_iterations(name, edge_floor, val6_floor):
    if name == "icosphere_q":
        v, f = synthetic.icosphere(6)
        v = synthetic.perturb(v.astype(F32), radial=0.02, seed=1).astype(F32)
    else:
        v, f = torus()
    h = F32(0.5 * avg_edge(v, f))
    V, F = rs.remesh_botsch(v, f, 5, h, True)
    L = np.linalg.norm(V[F[:, [1, 2, 0]]].astype(np.float64) - V[F], axis=2)
    assert ((L >= 0.8 * h) & (L <= 4 / 3 * h)).mean() >= edge_floor
    assert (rs.Topo(V, F).val == 6).mean() >= val6_floor


def test_projection_is_the_closest_point():
    v, f = MESHES["icosphere_perturbed"]
    rng = np.random.default_rng(0)
    p = v[rng.choice(v.shape[0], 50)] + rng.normal(scale=0.05, size=(50, 3)).astype(F32)
    q = rs.closest_points(p, v, f)
    d = np.linalg.norm(q - p, axis=1)
    # no triangle's dense sample is closer than the answer
    w = rng.dirichlet(np.ones(3), size=400)
    samples = np.einsum("sk,fkd->fsd", w, v[f].astype(np.float64)).reshape(-1, 3)
    dd = np.linalg.norm(p[:, None, :] - samples[None], axis=2).min(axis=1)
    assert (d <= dd + 1e-9).all()


def probe_points(v, f, n, seed):
    """points around a mesh: vertices and shared-edge midpoints exactly, and points near (0.02 of the box) and far (3 boxes) from it"""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    span = float(np.linalg.norm(v64.max(0) - v64.min(0)))
    e = edges(f)
    on_v = v64[rng.choice(v.shape[0], n)]
    on_e = e[rng.choice(e.shape[0], n)]
    on_e = (v64[on_e[:, 0]] + v64[on_e[:, 1]]) * 0.5
    near = v64[rng.choice(v.shape[0], n)] + rng.normal(scale=0.02 * span, size=(n, 3))
    far = rng.normal(scale=3.0 * span, size=(n, 3))
    return np.concatenate([on_v, on_e, near, far])


@pytest.mark.parametrize("name", ["icosphere_perturbed", "torus"])
def test_torch_closest_points_is_the_statement_bitwise(name):
    """closest_points_torch (the device brute force of the GPU tests) on torch CPU: the bits of closest_points, with chunk sizes that
    cut the triangle list inside vertex fans, so ties across chunks follow the first-minimum rule"""
    v, f = MESHES[name]
    p = probe_points(v, f, 60, seed=3)
    want = rs.closest_points(p, v, f)
    got, d2 = rs.closest_points_torch(p, v, f, "cpu", pchunk=97, tchunk=61)
    got = got.numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    dd = p - want
    assert np.array_equal(d2.numpy(), (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
    # through project(): the default and the torch port give the same vertices
    V, F, _ = rs.relax(v, f)
    a = rs.project(V, F, v, f)[0]
    b = rs.project(V, F, v, f, closest=rs.closest_on("cpu", pchunk=128, tchunk=100))[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
