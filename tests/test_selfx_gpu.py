"""
largesteps.distance's self-intersection queries on the device (csrc/selfx.hip) against tests/selfx_statement.py. The rule decides with
comparisons of fp64 numbers that the statement forms with the same operations in the same order, and the output is sorted, so the device
must return exactly the statement's array: no tolerance anywhere. Every mesh is small; icosphere(8) has 1280 faces, so that the walk
spans more than one workgroup of 256 leaves.
"""
import numpy as np
import pytest
import torch

import selfx_statement as sx
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def handle(v, f, dev, cls=None):
    from largesteps.distance import MeshDistance
    return (cls or MeshDistance)(*to(dev, v, f))


def degenerate():
    """the jittered icosphere(4) plus a zero-area face, repeated-index faces and a needle through the sphere"""
    v, f = sx.jittered(4, 1.0)
    k = v.shape[0]
    v = np.concatenate([v, F32([[0.0, 0.0, -2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 2.0], [0.01, 0.0, 2.0]])])
    extra = np.array([[k, k + 1, k + 2], [3, 3, 7], [5, 5, 5], [k, k + 2, k + 3], [k, k, k + 2]])      # collinear, repeated, a point, a needle, a segment
    return v, np.concatenate([f[:100], extra, f[100:]])


MESHES = sorted(sx.HAND_CASES) + ["ico4", "ico4_jittered", "two_spheres", "cutting_fold", "ico8_jittered", "degenerate", "single",
                                  "flat_sheet", "flat_sheet_rounded", "flat_sheet_pierced", "flat_sheet_far", "flat_overlap"]
_cache = {}


def mesh(name):
    """(V, F, the statement's IF), computed once per session; no test writes to them"""
    if name not in _cache:
        if name in sx.HAND_CASES:
            v, f = sx.hand_case(name)[:2]
        elif name == "ico4":
            v, f = synthetic.icosphere(4)
        elif name == "ico4_jittered":
            v, f = sx.jittered(4, 1.0)
        elif name == "two_spheres":
            v, f = sx.two_spheres()
        elif name == "cutting_fold":
            v, f = sx.cutting_fold()
        elif name == "ico8_jittered":
            v, f = sx.jittered(8, 1.0)
        elif name == "degenerate":
            v, f = degenerate()
        elif name == "flat_sheet":                  # the box clause (rule 3) decides these four
            v, f = sx.tilted_flat_sheet()
        elif name == "flat_sheet_rounded":
            v, f = sx.tilted_flat_sheet(12, 1.0 / 11.0)
        elif name == "flat_sheet_pierced":
            v, f = sx.pierced_flat_sheet()
        elif name == "flat_overlap":                # coplanar overlaps in a tilted plane: decided on rounding, near pairs kept
            v, f = sx.tilted_flat_overlap()
        elif name == "flat_sheet_far":              # an unreferenced vertex far away: e is 2^-40 x the largest coordinate of V
            v, f = sx.tilted_flat_sheet()
            v = np.concatenate([v, F32([[-4096.0, 0.0, 0.0]])])
        else:
            v, f = np.array([[0, 0, 0], [1, 0, 0], [0.25, 1, 0.5]], dtype=F32), np.array([[0, 1, 2]])
        f = np.asarray(f, dtype=np.int64)
        IF = sx.pairs_fast(v, f) if f.shape[0] > 700 else sx.pairs(v, f)          # test_selfx_cpu checks the filtered form on this mesh
        _cache[name] = (v, f, IF)
    return _cache[name]


@pytest.mark.parametrize("name", MESHES)
def test_the_device_returns_the_statements_pairs(dev, name):
    v, f, IF = mesh(name)
    with handle(v, f, dev) as m:
        got = m.self_intersections()
        cnt = m.count_self_intersections()
        faces = m.self_intersecting_faces()
    assert got.dtype == torch.int64 and got.device.type == "cuda" and tuple(got.shape) == (IF.shape[0], 2)
    assert np.array_equal(got.cpu().numpy(), IF), f"{name}: device {got.shape[0]} pairs, statement {IF.shape[0]}"
    assert cnt.dtype == torch.int64 and cnt.dim() == 0 and cnt.device.type == "cuda" and int(cnt) == IF.shape[0]
    mask = np.zeros(f.shape[0], dtype=bool)
    mask[IF.reshape(-1)] = True
    assert faces.dtype == torch.bool and np.array_equal(faces.cpu().numpy(), mask)


def test_expected_counts_of_the_named_meshes():
    """what the statement gives on the meshes above: the cases must stay cases"""
    for name in sorted(sx.HAND_CASES):
        assert mesh(name)[2].shape[0] == sx.HAND_CASES[name][2]
    assert mesh("ico4")[2].shape[0] == 0 and mesh("single")[2].shape[0] == 0
    assert mesh("ico4_jittered")[2].shape[0] == 230 and mesh("two_spheres")[2].shape[0] == 94 and mesh("cutting_fold")[2].shape[0] == 25
    v, f, IF = mesh("ico8_jittered")
    assert f.shape[0] == 1280 and IF.shape[0] > 256 and 0 < sx.shares_a_vertex(f, IF).sum() < IF.shape[0]
    for name, alone in (("flat_sheet", 205), ("flat_sheet_rounded", 6), ("flat_sheet_far", 205)):
        v, f, IF = mesh(name)                       # rule 2 alone accepts far-apart faces of the sheet on rounding; rule 3 leaves none
        fi, gi = np.triu_indices(f.shape[0], 1)
        assert sx.rule(v, f, fi, gi, box_clause=False).sum() == alone and IF.shape[0] == 0
    assert mesh("flat_sheet_pierced")[2].shape[0] > 0
    v, f, IF = mesh("flat_overlap")
    fi, gi = np.triu_indices(f.shape[0], 1)
    assert 0 < IF.shape[0] < sx.rule(v, f, fi, gi, box_clause=False).sum()
    v, f, IF = mesh("degenerate")
    # the needle cuts the sphere, and so do the edges of the collinear face and of the doubled segment (a zero-area face is never
    # crossed, but its edges are segments like any other); the face that is one point takes part in nothing
    assert all((IF == k).any() for k in (100, 103, 104)) and not (IF == 102).any()


def test_the_one_shot_forms_and_numpy_in_numpy_out(dev):
    from largesteps import distance
    v, f, IF = mesh("ico4_jittered")
    got = distance.self_intersections(v, f)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, IF)
    assert distance.count_self_intersections(v, f) == IF.shape[0] and isinstance(distance.count_self_intersections(v, f), int)
    found, faces = distance.fast_find_self_intersections(v, f)
    mask = np.zeros(f.shape[0], dtype=bool)
    mask[IF.reshape(-1)] = True
    assert found is True and isinstance(faces, np.ndarray) and faces.dtype == np.bool_ and np.array_equal(faces, mask)
    tv, tf = to(dev, v, f)
    got = distance.self_intersections(tv, tf.to(torch.int32))
    assert isinstance(got, torch.Tensor) and got.device == tv.device and np.array_equal(got.cpu().numpy(), IF)
    found, faces = distance.fast_find_self_intersections(tv, tf)
    assert found is True and faces.dtype == torch.bool and faces.device == tv.device
    v, f, _ = mesh("ico4")
    found, faces = distance.fast_find_self_intersections(v, f)
    assert found is False and not faces.any()
    got = distance.self_intersections(*to(dev, v, f))
    assert tuple(got.shape) == (0, 2) and got.dtype == torch.int64
    assert distance.self_intersections(v, f).shape == (0, 2)
    with distance.MeshDistance(*mesh("crossing")[:2]) as m:                       # a numpy handle
        assert isinstance(m.self_intersections(), np.ndarray) and m.count_self_intersections() == 1
        assert m.self_intersecting_faces().tolist() == [True, True]


def test_two_runs_give_identical_bits_and_ray_meshes_inherit(dev):
    from largesteps.raycast import RayMesh
    v, f, IF = mesh("ico8_jittered")
    with handle(v, f, dev) as a, handle(v, f, dev, RayMesh) as b:
        r1, r2, r3 = a.self_intersections(), a.self_intersections(), b.self_intersections()
        assert torch.equal(r1, r2) and torch.equal(r1, r3)
        assert torch.equal(a.self_intersecting_faces(), b.self_intersecting_faces())
        assert int(a.count_self_intersections()) == int(b.count_self_intersections()) == IF.shape[0]


def test_update_answers_as_a_fresh_handle(dev):
    v0, f, IF0 = mesh("ico4")
    v1, _, IF1 = mesh("ico4_jittered")
    with handle(v0, f, dev) as m:
        assert tuple(m.self_intersections().shape) == (0, 2)
        m.update(to(dev, v1)[0])
        assert np.array_equal(m.self_intersections().cpu().numpy(), IF1) and int(m.count_self_intersections()) == IF1.shape[0]
        with handle(v1, f, dev) as fresh:
            assert torch.equal(m.self_intersections(), fresh.self_intersections())
            assert torch.equal(m.self_intersecting_faces(), fresh.self_intersecting_faces())
        m.update(to(dev, v0)[0])
        assert int(m.count_self_intersections()) == 0 and not m.self_intersecting_faces().any()


def test_a_face_permutation_maps_the_result(dev):
    v, f, IF = mesh("ico8_jittered")
    perm = np.random.default_rng(7).permutation(f.shape[0])                       # new face j is old face perm[j]
    inv = np.argsort(perm)
    mapped = np.sort(inv[IF], axis=1)
    mapped = mapped[np.lexsort((mapped[:, 1], mapped[:, 0]))]
    with handle(v, f[perm], dev) as m:
        assert np.array_equal(m.self_intersections().cpu().numpy(), mapped)


def test_a_handle_keeps_the_kind_of_result_it_was_built_with(dev):
    """numpy or tensors out is decided at construction; `update` takes either and does not change it"""
    from largesteps.distance import MeshDistance
    v0, f, _ = mesh("ico4")
    v1, _, IF1 = mesh("ico4_jittered")
    with MeshDistance(v0, f) as m:                                                # built from numpy
        m.update(to(dev, v1)[0])
        got = m.self_intersections()
        assert isinstance(got, np.ndarray) and np.array_equal(got, IF1)
        assert isinstance(m.count_self_intersections(), int) and isinstance(m.self_intersecting_faces(), np.ndarray)
    with handle(v0, f, dev) as m:                                                 # built from tensors
        m.update(v1)
        got = m.self_intersections()
        assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), IF1)
        assert isinstance(m.count_self_intersections(), torch.Tensor) and isinstance(m.self_intersecting_faces(), torch.Tensor)


def test_a_workspace_that_is_too_small_is_refused(dev):
    import ctypes
    from largesteps import _native
    v, f, IF = mesh("ico4_jittered")
    k = IF.shape[0]
    need = ctypes.c_size_t(0)
    assert _native.lib().ls_mesh_selfx_workspace_bytes(f.shape[0], k, ctypes.byref(need)) == 0
    with handle(v, f, dev) as m:
        counts, total, _ = m._selfx_count(False)
        assert int(total) == k
        pairs = torch.full((k, 2), -1, dtype=torch.int64, device=dev)
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        args = (m._h, _native.ptr(counts), k, _native.ptr(pairs), _native.ptr(ws))
        st = _native.stream_of(m.device)
        for short in (0, need.value - 1):
            assert _native.lib().ls_mesh_selfx_pairs(*args, short, st) == _native.LS_E_WORKSPACE
            assert "workspace too small" in _native.last_error()
        torch.cuda.synchronize(dev)
        assert (pairs == -1).all()                                                # refused before anything was written
        assert _native.lib().ls_mesh_selfx_pairs(*args, need.value, st) == 0
        assert np.array_equal(pairs.cpu().numpy(), IF)


def test_a_closed_handle_raises(dev):
    v, f, _ = mesh("crossing")
    m = handle(v, f, dev)
    m.close()
    for call in (m.self_intersections, m.count_self_intersections, m.self_intersecting_faces):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_the_count_is_capturable_after_a_warm_up(dev):
    v, f, IF = mesh("ico4_jittered")
    with handle(v, f, dev) as m:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            m.count_self_intersections()                                          # the warm-up
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.count_self_intersections()
        out.zero_()
        graph.replay()
        assert int(out) == IF.shape[0]
        out.zero_()
        graph.replay()
        assert int(out) == IF.shape[0]
        del graph
