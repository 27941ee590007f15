"""
largesteps.remesh.remesh_botsch on the device (csrc/remesh.hip) against tests/remesh_statement.py: every phase on its own (identical
faces, positions within 2 ulp, int32 and int64 faces), single rounds at 70k, the full call (ls_remesh_run) on a grid of meshes and
settings with the handle's counters, the handle's runs and phases composed, the projection against a brute-force closest point on
meshes up to 1M vertices (folded sheets, a thin tube, graded and collapsed meshes, a mesh far from the origin), the full call on the
70k and 250k configs (invariants, reproducibility, numpy vs tensor entry, distance to the input surface), scripts/main.py's remesh
block end to end, and the argument errors.
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


# ---- the full call against the statement -----------------------------------------------------------------------------------------
def _ico(n):
    v, f = synthetic.icosphere(n)
    return synthetic.perturb(v, radial=0.05, seed=n).astype(F32), f


def translated(v, f):
    """the mesh moved to about 1000 diagonals from the origin (a part in scanner units): its coordinates' ulps exceed 1e-5 diagonals"""
    diag = float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0)))
    return (v.astype(np.float64) + 1000.0 * diag).astype(F32), f


def call_meshes():
    out = {f"ico{n}": _ico(n) for n in (6, 7, 8, 9, 12)}
    out["torus"] = torus()
    out["plane"] = synthetic.plane(10)
    sv, sf = out["ico6"]
    tv, tf = torus()
    out["sphere_torus"] = (np.concatenate([sv, tv + F32(3.0)]).astype(F32), np.concatenate([sf, tf + sv.shape[0]]))
    # 40 vertices no face references, before, among and after the used ones
    rng = np.random.default_rng(5)
    extra = np.sort(rng.choice(sv.shape[0] + 40, 40, replace=False))
    used = np.setdiff1d(np.arange(sv.shape[0] + 40), extra)
    uv = np.zeros((sv.shape[0] + 40, 3), F32)
    uv[used] = sv
    uv[extra] = rng.normal(size=(40, 3)).astype(F32)
    out["unreferenced"] = (uv, used[sf])
    out["translated"] = translated(sv, sf)
    return out


CALL_MESHES = call_meshes()

# every mesh, every h / avg in {0.15, 0.5, 1, 2, 4}, i in {0, 1, 5}, project on and off, int32 and int64 faces, numpy and tensor entry
CALLS = [("torus", 0.15, 1, True, np.int32, "tensor"), ("ico8", 0.5, 5, True, np.int64, "numpy"), ("ico12", 0.5, 5, True, np.int32, "tensor"),
         ("ico7", 2.0, 5, True, np.int64, "tensor"), ("ico6", 4.0, 5, True, np.int32, "numpy"), ("ico9", 1.0, 1, True, np.int64, "tensor"),
         ("ico7", 0.5, 5, False, np.int32, "tensor"), ("torus", 1.0, 5, False, np.int64, "tensor"), ("torus", 0.5, 0, True, np.int32, "numpy"),
         ("torus", 0.5, 5, True, np.int32, "tensor"), ("plane", 0.5, 5, True, np.int32, "numpy"), ("plane", 2.0, 1, False, np.int64, "tensor"),
         ("sphere_torus", 1.0, 5, True, np.int64, "tensor"), ("unreferenced", 0.5, 1, True, np.int32, "numpy"),
         ("unreferenced", 1.0, 0, False, np.int64, "tensor"), ("translated", 0.5, 5, True, np.int32, "tensor"),
         ("translated", 2.0, 1, False, np.int64, "numpy")]


@pytest.mark.parametrize("mesh,scale,iters,project,idx,entry", CALLS, ids=lambda x: getattr(x, "__name__", str(x)))
def test_full_call_matches_the_statement(dev, mesh, scale, iters, project, idx, entry):
    """remesh_botsch (ls_remesh_run: the iteration loop, the round caps, the buffers' growth over rounds, one BVH for all
    projections) against rs.remesh_botsch: identical faces, positions within 2 ulp, and the handle's round and operation counters
    equal to the statement's sums over the call"""
    from largesteps.remesh import RemeshHandle, remesh_botsch
    v, f = CALL_MESHES[mesh]
    h = F32(scale * avg_edge(v, f))
    stats = {}
    ev, ef = rs.remesh_botsch(v, f, iters, h, project, closest=rs.closest_on(dev), stats=stats)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(idx)).to(dev)
    if entry == "numpy":
        gv, gf = remesh_botsch(v.astype(np.float64), f.astype(idx), iters, h, project)
        assert gv.dtype == np.float64 and gf.dtype == np.int32
        gv = gv.astype(F32)
    else:
        tgv, tgf = remesh_botsch(tv, tf, iters, h, project)
        assert tgv.dtype == torch.float32 and tgf.dtype == tf.dtype
        gv, gf = tgv.cpu().numpy(), tgf.cpu().numpy()
    assert np.array_equal(gf.astype(np.int64), ef), "faces differ from the statement"
    assert gv.shape == ev.shape and ulps(gv, ev) <= 2
    with RemeshHandle(tv, tf, h, project) as r:
        r.run(iters)
        info = r.info()
        hv, hf = r.result()
    assert info["rounds"] == stats["rounds"] and info["ops"] == stats["ops"]
    assert np.array_equal(hf.cpu().numpy(), gf) and np.array_equal(hv.cpu().numpy().view(np.int32), gv.view(np.int32))


def _handle_state(r):
    V, F = r.result()
    return V.cpu().numpy().view(np.int32), F.cpu().numpy(), (r.info()["rounds"], r.info()["ops"])


def test_handle_runs_compose(dev):
    """run(2) then run(3) is run(5) bit for bit, counters included; the five phases called one by one are run(1)"""
    from largesteps.remesh import RemeshHandle
    v, f = CALL_MESHES["ico8"]
    h = F32(0.5 * avg_edge(v, f))
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    with RemeshHandle(tv, tf, h, True) as a, RemeshHandle(tv, tf, h, True) as b:
        a.run(5)
        b.run(2)
        b.run(3)
        sa, sb = _handle_state(a), _handle_state(b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]
    with RemeshHandle(tv, tf, h, True) as a, RemeshHandle(tv, tf, h, True) as b:
        a.run(1)
        for p, cap in (("split", rs.SPLIT_ROUNDS), ("collapse", rs.COLLAPSE_ROUNDS), ("flip", rs.FLIP_ROUNDS), ("relax", 1), ("project", 1)):
            b.phase(p, cap)
        sa, sb = _handle_state(a), _handle_state(b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]


def test_device_brute_force_is_the_statement_bitwise(dev):
    """closest_points_torch on the device gives the bits of numpy closest_points (so it may stand in for it below)"""
    from test_remesh_cpu import probe_points
    v, f = SMALL["torus"]
    p = probe_points(v, f, 64, seed=4)
    want = rs.closest_points(p, v, f)
    got, _ = rs.closest_points_torch(p, v, f, dev, pchunk=100, tchunk=70)
    assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))


# ---- single rounds at 70k --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bunny():
    v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    return v.astype(F32), f


@pytest.mark.parametrize("phase", ["split", "flip", "relax", "collapse"])
def test_one_round_at_scale_matches_the_statement(dev, bunny, phase):
    """one round on the 70k config (collapse: on a 10k-face sphere at h = 2 avg; the statement's collapse round takes minutes at 70k)"""
    v, f = bunny
    h = F32(0.5 * avg_edge(v, f))
    if phase == "flip":                      # an irregular input: one split round of the statement
        v, f, _ = rs.split_round(v, f, h)
    if phase == "collapse":
        v, f = _ico(22)
        h = F32(2.0 * avg_edge(v, f))
    fn = {"split": rs.split_round, "collapse": rs.collapse_round, "flip": rs.flip_round, "relax": rs.relax}[phase]
    ev, ef, n = fn(v, f, h)
    gv, gf, info = device_phase(dev, v, f, h, np.int32, [phase])
    if phase != "relax":
        assert n > (50 if phase == "collapse" else 1000), "the case must exercise the phase"
        assert info["ops"][phase] == n and info["rounds"][phase] == 1
    assert np.array_equal(gf, ef)
    assert gv.shape == ev.shape and ulps(gv, ev) <= 2


# ---- the projection at scale against the brute force ----------------------------------------------------------------------------
def tube(m=6000, k=12, radius=1e-3):
    """an open tube of length 1 and radius 1e-3 along x: m rings of k vertices"""
    x = np.arange(m) / (m - 1)
    w = np.arange(k) * 2 * np.pi / k
    X, W = np.meshgrid(x, w, indexing="ij")
    v = np.stack([X, radius * np.cos(W), radius * np.sin(W)], -1).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(m - 1), np.arange(k), indexing="ij")
    a, b, c, d = i * k + j, (i + 1) * k + j, (i + 1) * k + (j + 1) % k, i * k + (j + 1) % k
    return v, np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])


def projection_mesh(name):
    if name in ("cfg2_bunny70k", "cfg3_dragon250k", "cfg4b_sphere1m"):
        v, f, _ = synthetic.config_mesh(name)
    elif name == "folded":
        v, f = synthetic.folded_sheet(120)
    elif name == "scroll":
        v, f = synthetic.scroll(120, 10)
    elif name == "shells":
        v, f = synthetic.shells(40)
    elif name == "tube":
        v, f = tube()
    elif name in ("graded", "collapsed"):
        from test_ordering_cpu import _hard_mesh
        v, f = _hard_mesh(name)
    else:
        v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
        v, f = translated(v.astype(F32), f)
    v, f = np.asarray(v, dtype=F32), np.asarray(f, dtype=np.int64)
    rs.validate(v, f)
    return v, f


PROJECTION_MESHES = {"cfg2_bunny70k": None, "folded": None, "scroll": None, "shells": None, "cfg3_dragon250k": 16384,
                     "cfg4b_sphere1m": 16384, "tube": None, "graded": None, "collapsed": None, "bunny_translated": None}


@pytest.mark.parametrize("iters", [0, 4])
@pytest.mark.parametrize("name", list(PROJECTION_MESHES))
def test_projection_is_the_brute_force_closest_point(dev, name, iters):
    """after run(iters), split / collapse / flip to their caps and relax: the projection moves every interior vertex to the fp32
    rounding of the brute-force fp64 closest point of its pre-projection position (the LBVH walk prunes nothing it should not), and
    its fp64 squared distance is at most the brute-force minimum plus the slack of that rounding. The fp64 test is the statement's
    and the tie rule the same, so the answer is exact: the same bits, not only within 2 ulp. On the largest meshes: a fixed sample of
    the interior vertices and the 1024 that relax moved most."""
    from largesteps.remesh import RemeshHandle
    v, f = projection_mesh(name)
    avg = avg_edge(v, f)
    h = F32(0.5 * avg) if avg > 0 else F32(1e-2)
    with RemeshHandle(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), h, True) as r:
        r.run(iters)
        for p, cap in (("split", rs.SPLIT_ROUNDS), ("collapse", rs.COLLAPSE_ROUNDS), ("flip", rs.FLIP_ROUNDS)):
            r.phase(p, cap)
        P_flip, _ = r.result()
        r.phase("relax")
        P_pre, F_pre = r.result()
        r.phase("project")
        P_post, F_post = r.result()
    assert torch.equal(F_pre, F_post)
    F_np = F_post.cpu().numpy().astype(np.int64)
    t = rs.Topo(np.zeros((P_post.shape[0], 3), F32), F_np)
    interior = np.nonzero(~t.bnd & (t.cnt > 0))[0]
    pre, post = P_pre.cpu().numpy(), P_post.cpu().numpy()
    fixed = np.setdiff1d(np.arange(pre.shape[0]), interior)
    assert np.array_equal(pre[fixed].view(np.int32), post[fixed].view(np.int32)), "a boundary vertex moved"
    idx = interior
    sample = PROJECTION_MESHES[name]
    if sample is not None and interior.size > sample:
        moved = torch.linalg.vector_norm((P_pre - P_flip).double(), dim=1).cpu().numpy()[interior]
        top = interior[np.argsort(-moved, kind="stable")[:1024]]
        rng = np.random.default_rng(0)
        idx = np.union1d(rng.choice(interior, sample, replace=False), top)
    q, d2 = rs.closest_points_torch(torch.from_numpy(pre[idx]), v, f, dev, pchunk=256, tchunk=65536)
    want = q.float().cpu().numpy()
    got = post[idx]
    n_off = int((got.view(np.int32) != want.view(np.int32)).any(axis=1).sum())
    assert n_off == 0, f"{n_off} of {idx.size} vertices are not the brute force's (largest difference {ulps(got, want)} ulp)"
    e = torch.linalg.vector_norm(q - q.float().double(), dim=1)
    dpost = ((torch.from_numpy(post[idx]).to(dev).double() - torch.from_numpy(pre[idx]).to(dev).double()) ** 2).sum(1)
    bound = (torch.sqrt(d2) + e) ** 2 * (1 + 1e-12)
    assert bool((dpost <= bound).all()), "a vertex is farther from the input surface than the brute force's nearest point"
