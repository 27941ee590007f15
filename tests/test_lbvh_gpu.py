"""
The build of csrc/lbvh.h on the device against tests/lbvh_statement.py, at the codes the query suites never produce: every face in one
Morton cell, runs of equal codes of many lengths, trees of 1 to 5 leaves and of one leaf either side of a workgroup, an axis of zero
extent, a handle rebuilt in place between all-distinct and all-equal codes, a NaN in the mesh. The arrays the device exports (left,
right, esc, tri, box) must be the statement's, the boxes bit for bit. Then the answers of the five query families on trees whose boxes
separate nothing, each against its own statement and with its own helper: the ties that go to the lowest face id have only been
tested where the hierarchy happened to keep the candidates apart.
"""
import numpy as np
import pytest
import torch

import lbvh_statement as lb
import ray_statement as rs
import selfx_statement as sx
import winding_statement as ws

pytestmark = pytest.mark.gpu
F32 = np.float32
ANSWER_CASES = ["far4096", "far320", "far_face", "repeated"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def handle(v, f, dev, cls=None):
    from largesteps.distance import MeshDistance
    return (cls or MeshDistance)(*to(dev, v, f))


def export(m):
    """left, right, esc, tri and box of a handle, in the statement's format; no moments are asked for or prepared"""
    from largesteps import _native
    T = m._f.shape[0]
    N = 2 * T - 1
    i32 = dict(dtype=torch.int32, device=m.device)
    left, right, esc, tri = torch.zeros(max(T - 1, 1), **i32), torch.zeros(max(T - 1, 1), **i32), torch.zeros(N, **i32), torch.zeros(T, **i32)
    box = torch.zeros((N, 6), dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        _native.check(_native.lib().ls_mesh_winding_arrays(m._h, None, _native.ptr(left), _native.ptr(right), _native.ptr(esc), _native.ptr(tri),
                                                           _native.ptr(box), None, _native.stream_of(m.device)))
        torch.cuda.synchronize(m.device)
    return dict(left=left.cpu().numpy()[:T - 1], right=right.cpu().numpy()[:T - 1], esc=esc.cpu().numpy(), tri=tri.cpu().numpy(), box=box.cpu().numpy())


def check_arrays(got, v, f, what):
    """the invariants first, so that a failure names the property; then the statement, exactly"""
    lb.check_invariants(got)
    want = lb.build(v, f)
    diff = lb.differing(want, got)
    assert not diff, f"{what}: {diff} differ from the statement"
    return want


# ---- the arrays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lb.CASES)
def test_the_devices_arrays_are_the_statements(dev, name):
    v, f = lb.case(name)
    with handle(v, f, dev) as m:
        got = export(m)
    want = check_arrays(got, v, f, name)
    r = lb.runs(want["code"])
    print(f"{name}: T = {f.shape[0]}, {len(r)} distinct codes, longest run {r.max()}, depth {lb.depth(want)}")


@pytest.mark.parametrize("name", ["far320", "far_face"])
def test_int32_and_int64_faces_build_the_same_arrays(dev, name):
    v, f = lb.case(name)
    with handle(v, f.astype(np.int32), dev) as a, handle(v, f.astype(np.int64), dev) as b:
        ga, gb = export(a), export(b)
    check_arrays(ga, v, f, name + ", int32 faces")
    check_arrays(gb, v, f, name + ", int64 faces")


def test_a_rebuild_in_place_moves_between_distinct_and_equal_codes(dev):
    """update() reuses parent and rflag after a memset: the tree of all-equal codes must not show through the next one, nor the reverse"""
    v, f = lb.sphere()
    pos = lb.with_far_vertex(v, 0.0)
    distinct = []
    with handle(pos, f, dev) as m:
        check_arrays(export(m), pos, f, "as built")
        for s in (1.0, 4096.0, 320.0, 1.0):
            pos = lb.with_far_vertex(v, s)
            m.update(to(dev, pos)[0])
            got = export(m)
            want = check_arrays(got, pos, f, f"after update to x{s:g}")
            with handle(pos, f, dev) as fresh:
                assert not lb.differing(export(fresh), got), f"x{s:g}: the updated handle and a fresh one differ"
            distinct.append(len(lb.runs(want["code"])))
    assert distinct == [720, 1, 169, 720]


# ---- the answers on trees that prune nothing or split oddly ------------------------------------------------------------------------------
def query_source(name):
    """the mesh the query generators see: the referenced vertices only. `probes`, `rays` and `queries` scale by the vertex box, and
    with the far vertex in it nearly every ray would miss"""
    v, f = lb.sphere()
    if name == "repeated":
        return np.ascontiguousarray(v[f[0]]), np.array([[0, 1, 2]])
    return v, f


_rays = {}
# a single triangle is hit by about a fifth of the rays of test_raycast_gpu.rays, 19 to 21 % with the seed; its own single-face case has
# seed 6 and meets its guard (more than a fifth hit), so the repeated face takes that seed. test_lbvh_statement_cpu checks the guard
RAY_SEED = {"far4096": 0, "far320": 1, "far_face": 2, "repeated": 6, "nan": 4}


def ray_case(name, dev):
    """(v, f, O, D, trange, the statement's (t, I, W)) as test_raycast_gpu.case gives them; `dev` may be the CPU"""
    from test_raycast_gpu import rays, with_ranges
    key = (name, str(dev))
    if key not in _rays:
        v, f = lb.case(name)
        O, D = rays(*query_source(name), seed=RAY_SEED[name])
        O, D, tr = with_ranges(O, D, v, f, dev)
        want = tuple(x.cpu().numpy() for x in rs.closest_torch(O, D, v, f, tr, dev, chunk=256))
        _rays[key] = (v, f, O, D, tr, want)
    return _rays[key]


@pytest.mark.parametrize("name", ANSWER_CASES)
def test_the_distance_is_the_statement_bitwise(dev, name):
    from test_distance_gpu import check_against_statement, probes
    v, f = lb.case(name)
    d2, I, C = check_against_statement(dev, v, f, probes(*query_source(name), 128, seed=ANSWER_CASES.index(name)))
    if name == "repeated":
        assert not bool(I.any())                             # 300 faces tie everywhere: the lowest id
    else:
        assert int(I.unique().numel()) > 100


@pytest.mark.parametrize("name", ANSWER_CASES)
def test_the_rays_are_the_statement_bitwise(dev, name):
    from test_raycast_gpu import check_against_statement
    v, f, O, D, tr, (t, I, W) = check_against_statement(dev, name, given=ray_case(name, dev))
    if name == "repeated":
        assert (I[I >= 0] == 0).all()


@pytest.mark.parametrize("beta", [2.0, 1e30])
@pytest.mark.parametrize("name", ANSWER_CASES)
def test_the_winding_walk_is_the_statements_walk(dev, name, beta):
    from test_winding_cpu import queries, tol
    from test_winding_gpu import export as export_with_moments
    v, f = lb.case(name)
    T = f.shape[0]
    P, _ = queries(*query_source(name), seed=20 + ANSWER_CASES.index(name))
    with handle(v, f, dev) as m:
        arrays, mom = export_with_moments(m)
        got = m.winding_number(to(dev, P)[0], beta=beta).cpu().numpy()
    want, s, acc, leaves = ws.walk(P, arrays, mom, beta)
    err = np.abs(got - want)
    print(f"{name}, beta {beta:g}: largest deviation {err.max():.2e} (allowed from {tol(T, s).min():.2e}); {acc.mean():.0f} nodes accepted, "
          f"{leaves.mean():.0f} leaves per query")
    assert np.isfinite(want).all() and (err <= tol(T, s)).all()
    if beta == 1e30:
        assert (acc == 0).all() and (leaves == T).all()


_selfx = {}


def selfx_case(name):
    """(V, F, the statement's pairs), once"""
    if name not in _selfx:
        if name == "repeated":
            v, f = lb.case(name)
        elif name == "nan":
            v, f = lb.case(name)
        else:
            v, f = sx.jittered(4, 1.0)                       # test_selfx_gpu's ico4_jittered: 320 faces, 230 pairs
            if name == "nan_jittered":
                v = v.copy()
                v[f[100, 1], 0] = np.nan
            else:
                v = lb.with_far_vertex(v, float(name[len("jittered_far"):]))
        _selfx[name] = (v, f, sx.pairs(v, f))
    return _selfx[name]


@pytest.mark.parametrize("name", ["jittered_far4096", "jittered_far320", "repeated"])
def test_the_self_intersections_are_the_statements_pairs(dev, name):
    v, f, IF = selfx_case(name)
    assert (IF.shape[0] == 0) == (name == "repeated")        # all index triples coincide there: s = 3, never reported
    with handle(v, f, dev) as m:
        got = m.self_intersections().cpu().numpy()
        cnt = int(m.count_self_intersections())
    assert np.array_equal(got, IF) and cnt == IF.shape[0], f"{name}: device {got.shape[0]} pairs, statement {IF.shape[0]}"


# ---- a NaN in the mesh -----------------------------------------------------------------------------------------------------------------
def test_a_nan_vertex_keeps_the_tree_valid_and_the_rays_exact(dev):
    """a non-finite coordinate costs time, not correctness (DESIGN.md sections 2.10 and 2.12): the faces around the vertex are never hit,
    every other ray answers as the brute force does"""
    from largesteps.raycast import RayMesh
    from test_raycast_gpu import check_against_statement
    v, f = lb.case("nan")
    with handle(v, f, dev, RayMesh) as m:
        got = export(m)
    check_arrays(got, v, f, "nan")
    v, f, O, D, tr, (t, I, W) = check_against_statement(dev, "nan", given=ray_case("nan", dev))
    bad = int(np.nonzero(np.isnan(v).any(1))[0][0])
    around = np.nonzero((f == bad).any(1))[0]
    assert around.size >= 5 and not np.isin(I, around).any()
    assert np.isfinite(W).all() and not np.isnan(t).any()


@pytest.mark.parametrize("name", ["nan", "nan_jittered"])
def test_a_nan_vertex_leaves_the_self_intersections_the_statements(dev, name):
    v, f, IF = selfx_case(name)
    assert np.isnan(v).sum() == 1 and (name == "nan" or IF.shape[0] > 0)
    with handle(v, f, dev) as m:
        lb.check_invariants(export(m))
        got = m.self_intersections().cpu().numpy()
        faces = m.self_intersecting_faces().cpu().numpy()
    assert np.array_equal(got, IF), f"{name}: device {got.shape[0]} pairs, statement {IF.shape[0]}"
    mask = np.zeros(f.shape[0], dtype=bool)
    mask[IF.reshape(-1)] = True
    assert np.array_equal(faces, mask)
