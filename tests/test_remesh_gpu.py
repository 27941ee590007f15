"""
largesteps.remesh.remesh_botsch on the device (csrc/remesh.hip) against tests/remesh_statement.py: every phase on its own (identical
faces, positions within 2 ulp, int32 and int64 faces), the full call on the 70k and 250k configs (invariants, reproducibility,
numpy vs tensor entry, distance to the input surface), scripts/main.py's remesh block end to end, and the argument errors.
"""
import numpy as np
import pytest
import torch

import remesh_statement as rs
from test_remesh_cpu import avg_edge, check_invariants, torus
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def ulps(a, b):
    """largest distance in units in the last place between two fp32 arrays (signed zeros equal)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max(initial=0))


def small_meshes():
    v, f = synthetic.icosphere(6)
    return {"ico": (synthetic.perturb(v, radial=0.05, seed=2).astype(F32), f), "plane": synthetic.plane(10), "torus": torus()}


SMALL = small_meshes()


def device_phase(dev, v, f, h, idx, phases):
    from largesteps.remesh import RemeshHandle
    with RemeshHandle(torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(idx)).to(dev), h, True) as r:
        for p in phases:
            r.phase(p, 1)
        V, F = r.result()
        assert F.dtype == torch.from_numpy(np.zeros(1, idx)).dtype
        return V.cpu().numpy(), F.cpu().numpy().astype(np.int64), r.info()


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("mesh", sorted(SMALL))
@pytest.mark.parametrize("phase,scale", [("split", 0.5), ("collapse", 2.0), ("flip", 0.5), ("relax", 1.0), ("project", 1.0)])
def test_each_phase_matches_the_statement(dev, mesh, phase, scale, idx):
    v, f = SMALL[mesh]
    h = F32(scale * avg_edge(v, f))
    if phase == "flip":                      # an irregular input: two split rounds of the statement
        hs = F32(0.4 * avg_edge(v, f))
        v, f, _ = rs.split_round(*rs.split_round(v, f, hs)[:2], hs)
    V0, F0 = v, f
    if phase == "project":                   # relax moves the vertices off the surface, project brings them back
        ev, ef, _ = rs.relax(v, f)
        ev, ef, _ = rs.project(ev, ef, V0, F0)
        gv, gf, _ = device_phase(dev, v, f, h, idx, ["relax", "project"])
    else:
        fn = {"split": rs.split_round, "collapse": rs.collapse_round, "flip": rs.flip_round, "relax": rs.relax}[phase]
        ev, ef, n = fn(v, f, h)
        if phase != "relax":
            assert n > 0, "the case must exercise the phase"
        gv, gf, info = device_phase(dev, v, f, h, idx, [phase])
        if phase != "relax":
            assert info["ops"][phase] == n
    assert np.array_equal(gf, ef)
    assert gv.shape == ev.shape and ulps(gv, ev) <= 2


def test_phase_fixpoints_match_the_statement(dev):
    """several rounds of each phase (the round loop and its stop rule) on the perturbed sphere"""
    from largesteps.remesh import RemeshHandle
    v, f = SMALL["ico"]
    h = F32(0.5 * avg_edge(v, f))
    ev, ef = v, f
    with RemeshHandle(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), h, True) as r:
        for p, fn, cap in (("split", rs.split_round, rs.SPLIT_ROUNDS), ("collapse", rs.collapse_round, rs.COLLAPSE_ROUNDS),
                           ("flip", rs.flip_round, rs.FLIP_ROUNDS)):
            ev, ef, rounds, ops = rs.run_phase(fn, cap, ev, ef, h)
            r.phase(p, cap)
            info = r.info()
            assert info["rounds"][p] == rounds and info["ops"][p] == ops
        gv, gf = r.result()
    assert np.array_equal(gf.cpu().numpy(), ef) and ulps(gv.cpu().numpy(), ev) <= 2


def point_triangle_distance(p, a, b, c):
    """(P, T) distances of points p (P, 3) to triangles (T, 3) each, fp32 on the device (brute force)"""
    p = p[:, None, :]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    den = 1.0 / (va + vb + vc)
    r = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    r = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None], r)
    r = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * (d2 / (d2 - d6))[..., None], r)
    r = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c.expand_as(r), r)
    r = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * (d1 / (d1 - d3))[..., None], r)
    r = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b.expand_as(r), r)
    r = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a.expand_as(r), r)
    return (p - r).norm(dim=-1)


def surface_distance(P, V0, F0, chunk=256):
    a, b, c = (V0[F0[:, k]][None] for k in range(3))
    out = []
    for s in range(0, P.shape[0], chunk):
        out.append(point_triangle_distance(P[s:s + chunk], a, b, c).min(dim=1).values)
    return torch.cat(out)


@pytest.fixture(scope="module", params=["cfg2_bunny70k", "cfg3_dragon250k"])
def big(request, dev):
    from largesteps.meshops import average_edge_length
    from largesteps.remesh import remesh_botsch
    v, f, _ = synthetic.config_mesh(request.param)
    tv, tf = torch.from_numpy(v.astype(F32)).to(dev), torch.from_numpy(f).to(dev)
    h = average_edge_length(tv, tf) * 0.5
    V1, F1 = remesh_botsch(tv, tf, 5, h, True)
    V2, F2 = remesh_botsch(tv, tf, 5, h, True)
    Vn, Fn = remesh_botsch(v.astype(np.float64), f.astype(np.int32), 5, h.cpu().numpy(), True)
    return dict(name=request.param, v=v.astype(F32), f=f, tv=tv, tf=tf, h=float(h), out=(V1, F1), again=(V2, F2), numpy=(Vn, Fn))


def test_full_remesh_invariants_and_reproducibility(big):
    V1, F1 = big["out"]
    assert V1.dtype == torch.float32 and F1.dtype == big["tf"].dtype and V1.device == big["tv"].device
    v, f = V1.cpu().numpy(), F1.cpu().numpy()
    check_invariants(big["v"], big["f"], v, f)
    assert f.shape[0] != big["f"].shape[0]
    V2, F2 = big["again"]
    assert torch.equal(F1, F2) and torch.equal(V1.view(torch.int32), V2.view(torch.int32)), "two calls differ"
    Vn, Fn = big["numpy"]
    assert Vn.dtype == np.float64 and Fn.dtype == np.int32
    assert np.array_equal(Fn, f) and np.array_equal(Vn.astype(F32).view(np.int32), v.view(np.int32)), "numpy and tensor entries differ"


def test_full_remesh_stays_on_the_input_surface(big):
    V1, _ = big["out"]
    V0, F0 = big["tv"], big["tf"]
    diag = float((V0.max(0).values - V0.min(0).values).norm())
    P = V1
    if big["name"] == "cfg3_dragon250k":
        g = torch.Generator().manual_seed(0)
        P = V1[torch.randperm(V1.shape[0], generator=g)[:2000].to(V1.device)]
    d = surface_distance(P, V0, F0.long())
    assert float(d.max()) <= 1e-5 * diag


def test_main_py_remesh_block(dev):
    """scripts/main.py:146-163 on the 70k config: remesh, remove_duplicates, compute_matrix -> to_differential -> from_differential"""
    from largesteps.geometry import compute_matrix
    from largesteps.meshops import average_edge_length, remove_duplicates
    from largesteps.parameterize import from_differential, to_differential
    from largesteps.remesh import remesh_botsch
    from oracle import solve as osv
    v, f, cfg = synthetic.config_mesh("cfg2_bunny70k")
    v_unique, f_unique = torch.from_numpy(v.astype(F32)).to(dev), torch.from_numpy(f).to(dev)
    h = (average_edge_length(v_unique, f_unique)).cpu().numpy() * 0.5
    v_new, f_new = remesh_botsch(v_unique.cpu().numpy().astype(np.double), f_unique.cpu().numpy().astype(np.int32), 5, h, True)
    v_src = torch.from_numpy(v_new).cuda().float().contiguous()
    f_src = torch.from_numpy(f_new).cuda().contiguous()
    v_unique, f_unique, duplicate_idx = remove_duplicates(v_src, f_src)
    assert v_unique.shape[0] == v_src.shape[0], "the remesher produced duplicate vertices"
    M = compute_matrix(v_unique, f_unique, lambda_=cfg["lambda_"])
    u = to_differential(M, v_unique)
    x = from_differential(M, u, "Cholesky")
    idx, val = M.indices().cpu().numpy(), M.values().cpu().numpy()
    x64 = osv.from_differential(idx[0], idx[1], val, u.cpu().numpy())
    assert np.abs(x.cpu().numpy() - x64).max() <= 1e-4 * np.abs(x64).max()


def test_argument_errors(dev):
    from largesteps import normals
    from largesteps.remesh import remesh_botsch
    v, f = synthetic.icosphere(3)
    tv, tf = torch.from_numpy(v.astype(F32)), torch.from_numpy(f)
    with pytest.raises(RuntimeError) as ours:
        remesh_botsch(tv, tf, 1, 0.1, True)
    with pytest.raises(RuntimeError) as theirs:
        normals.compute_face_normals(tv, tf.T.contiguous())
    assert type(ours.value) is type(theirs.value) and "no CPU path" in str(ours.value) and "no CPU path" in str(theirs.value)
    with pytest.raises(TypeError):
        remesh_botsch(tv.double().to(dev), tf.to(dev), 1, 0.1, True)
    with pytest.raises(TypeError):
        remesh_botsch(tv.to(dev), tf.float().to(dev), 1, 0.1, True)
    g = f.copy()
    g[0] = g[0, ::-1]
    with pytest.raises(ValueError):
        remesh_botsch(tv.to(dev), torch.from_numpy(g).to(dev), 1, 0.1, True)
    with pytest.raises(ValueError):
        remesh_botsch(v.astype(np.float64), np.concatenate([f, [[0, 0, 1]]]).astype(np.int32), 1, 0.1, True)
