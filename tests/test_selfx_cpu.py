"""
The self-intersection query of largesteps.distance without a device: the rule of tests/selfx_statement.py on hand cases whose answer is
known and on the meshes of the device tests (with the counts of the prototype the rule was chosen from), the box-filtered form against
the brute force, the invariances of the pair set, and the public surface with the argument errors that come before any device work.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import selfx_statement as sx
from largesteps import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def jit4():
    v, f = sx.jittered(4, 1.0)
    return v, f, sx.pairs(v, f)


@pytest.mark.parametrize("name", sorted(sx.HAND_CASES))
def test_hand_cases(name):
    v, f, k = sx.hand_case(name)
    IF = sx.pairs(v, f)
    assert IF.shape == (k, 2) and IF.dtype == np.int64 and (IF[:, 0] < IF[:, 1]).all()
    assert np.array_equal(sx.pairs_fast(v, f), IF)


def test_the_segment_rule_on_its_boundaries():
    a, b, c = [0, 0, 0], [2, 0, 0], [0, 2, 0]
    assert sx.crosses([0.5, 0.5, -1], [0.5, 0.5, 1], a, b, c)
    assert sx.crosses([0.5, 0.5, 1], [0.5, 0.5, 0], a, b, c) and sx.crosses([0.5, 0.5, 0], [0.5, 0.5, 1], a, b, c)      # t = 1 and t = 0
    assert not sx.crosses([0.5, 0.5, 1], [0.5, 0.5, 0.25], a, b, c)                                                  # stops short
    assert sx.crosses([1, 0, -1], [1, 0, 1], a, b, c) and sx.crosses([0, 0, -1], [0, 0, 1], a, b, c)                      # an edge, a vertex
    assert not sx.crosses([0.5, 0.5, 0], [1.5, 0.25, 0], a, b, c)                                                    # in the plane: det == 0
    assert not sx.crosses([0.5, 0.5, -1], [0.5, 0.5, 1], a, b, b) and not sx.crosses([0.5, 0.5, -1], [0.5, 0.5, 1], a, a, a)   # zero area
    assert not sx.crosses([0.5, 0.5, 1], [0.5, 0.5, 1], a, b, c)                                                     # d == 0
    assert not sx.crosses([0.5, 0.5, -1], [0.5, 0.5, np.inf], a, b, c) and not sx.crosses([np.nan, 0.5, -1], [0.5, 0.5, 1], a, b, c)


def test_a_clean_sphere_has_none_and_mild_noise_keeps_it_so():
    v, f = synthetic.icosphere(8)
    assert f.shape[0] == 1280
    assert sx.pairs(v, f).shape == (0, 2) and sx.pairs_fast(v, f).shape == (0, 2)
    for n in (2, 4):
        v, f = synthetic.icosphere(n)
        assert sx.pairs(v, f).shape == (0, 2)
        assert sx.pairs(*sx.jittered(n, 0.2)).shape == (0, 2)
        assert sx.pairs(synthetic.perturb(v, radial=0.02, seed=5).astype(F32), f).shape == (0, 2)


def test_the_jittered_sphere_has_pairs_of_both_classes(jit4):
    v, f, IF = jit4
    shared = sx.shares_a_vertex(f, IF)
    print(f"icosphere(4), jitter 1.0: {IF.shape[0]} pairs, {int(shared.sum())} of them share a vertex")
    assert (~shared).sum() > 0 and shared.sum() > 0
    assert (IF.shape[0], int(shared.sum())) == (230, 84)                      # the prototype's counts
    assert np.array_equal(sx.pairs_fast(v, f), IF)
    assert (IF[:, 0] < IF[:, 1]).all() and (np.diff(IF[:, 0] * f.shape[0] + IF[:, 1]) > 0).all()      # sorted, no pair twice
    # no reported pair shares an edge
    assert ((f[IF[:, 0]][:, :, None] == f[IF[:, 1]][:, None, :]).sum((1, 2)) <= 1).all()


def test_two_spheres_the_cutting_fold_and_the_flat_fold():
    v, f = sx.two_spheres()
    IF = sx.pairs(v, f)
    assert IF.shape[0] == 94 and np.array_equal(sx.pairs_fast(v, f), IF)
    assert (IF[:, 0] < 320).all() and (IF[:, 1] >= 320).all()                 # every pair has a face of either sphere
    v, f = sx.cutting_fold()
    IF = sx.pairs(v, f)
    assert IF.shape[0] == 25 and np.array_equal(sx.pairs_fast(v, f), IF)
    for gap in (0.0, 1e-3):                                                   # folded flat: coplanar or apart, never reported
        v, f = synthetic.folded_sheet(12, gap=gap)
        assert sx.pairs(v, f).shape == (0, 2)


def all_pairs(f):
    return np.triu_indices(f.shape[0], 1)


@pytest.mark.parametrize("step, alone", [(1.0 / 16.0, 205), (1.0 / 11.0, 6)])
def test_the_box_clause_decides_a_flat_tilted_sheet(step, alone):
    """an exactly flat sheet whose shear rounds: rule 2 alone accepts faces lattice steps apart (U = W = 0, det = V = a rounding error),
    rule 3 leaves none of them, in the brute force and in the filtered form alike"""
    v, f = sx.tilted_flat_sheet(12, step)
    assert f.shape[0] == 242
    if step == 1.0 / 16.0:
        assert np.array_equal(v.astype(np.float64)[:, 2], v.astype(np.float64)[:, 0] + 3.0 * v.astype(np.float64)[:, 1])       # exactly flat
    fi, gi = all_pairs(f)
    rep = sx.rule(v, f, fi, gi, box_clause=False)
    assert rep.sum() == alone
    assert not sx.boxes_near(v, f, fi[rep], gi[rep]).any()                   # every one of them has boxes apart ...
    lo, hi = v[f].min(1).astype(np.float64), v[f].max(1).astype(np.float64)
    gap = np.maximum(lo[gi[rep]] - hi[fi[rep]], lo[fi[rep]] - hi[gi[rep]]).max(1)
    assert (gap > 1e-3).all() and sx.slack(v) < 1e-11                         # ... by a lattice step or so, not by a rounding
    assert sx.pairs(v, f).shape == (0, 2) and sx.pairs_fast(v, f).shape == (0, 2)


def test_the_box_clause_changes_nothing_where_faces_really_cross(jit4):
    for v, f, IF in (jit4, sx.cutting_fold() + (None,), sx.two_spheres() + (None,)):
        fi, gi = all_pairs(f)
        rep = sx.rule(v, f, fi, gi, box_clause=False)
        assert np.array_equal(np.stack([fi[rep], gi[rep]], 1), sx.pairs(v, f) if IF is None else IF)


def test_a_pierced_flat_sheet_keeps_the_piercing_pairs_only():
    v, f = sx.pierced_flat_sheet()
    IF = sx.pairs(v, f)
    assert IF.shape[0] > 0 and (IF[:, 1] == f.shape[0] - 1).all() and np.array_equal(sx.pairs_fast(v, f), IF)
    fi, gi = all_pairs(f)
    assert sx.rule(v, f, fi, gi, box_clause=False).sum() > IF.shape[0]


def test_a_coplanar_overlap_in_a_tilted_plane_is_decided_the_same_way_by_both_forms():
    v, f = sx.tilted_flat_overlap()
    z = v.astype(np.float64)
    assert np.array_equal(z[:, 2], z[:, 0] + 3.0 * z[:, 1])                   # exactly flat
    IF = sx.pairs(v, f)
    fi, gi = all_pairs(f)
    assert 0 < IF.shape[0] < sx.rule(v, f, fi, gi, box_clause=False).sum() and np.array_equal(sx.pairs_fast(v, f), IF)


def test_the_filtered_form_is_the_brute_force_on_a_larger_jittered_sphere():
    v, f = sx.jittered(8, 1.0)
    IF = sx.pairs_fast(v, f)
    assert IF.shape[0] > 0 and np.array_equal(IF, sx.pairs(v, f))


def as_set(IF):
    return set(map(tuple, IF.tolist()))


def test_renumbering_the_faces_maps_the_pair_set(jit4):
    v, f, IF = jit4
    perm = np.random.default_rng(3).permutation(f.shape[0])                   # new face j is old face perm[j]
    inv = np.argsort(perm)
    got = sx.pairs(v, f[perm])
    mapped = np.sort(inv[IF], axis=1)
    assert as_set(got) == as_set(mapped) and got.shape[0] == IF.shape[0]


def test_rotating_and_reversing_corners_keeps_the_pair_set(jit4):
    v, f, IF = jit4
    rng = np.random.default_rng(4)
    shift = rng.integers(0, 3, f.shape[0])
    rot = np.stack([f[np.arange(f.shape[0]), (shift + k) % 3] for k in range(3)], 1)
    assert np.array_equal(sx.pairs(v, rot), IF)
    flip = np.where(rng.integers(0, 2, f.shape[0])[:, None] == 1, f[:, ::-1], f)
    assert np.array_equal(sx.pairs(v, flip), IF)


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_the_module_has_the_documented_symbols():
    from largesteps import distance, raycast
    for name in ("count_self_intersections", "self_intersecting_faces", "self_intersections"):
        method = getattr(distance.MeshDistance, name)
        assert list(inspect.signature(method).parameters) == ["self"]
        assert getattr(raycast.RayMesh, name) is method
        assert "ot differentiable" in method.__doc__
    for name in ("self_intersections", "count_self_intersections", "fast_find_self_intersections"):
        assert list(inspect.signature(getattr(distance, name)).parameters) == ["V", "F"]
    for words in ("oplanar overlaps are not reported", "share no index", "remove_duplicates", "at least one of them"):
        assert words in distance.__doc__, words


def test_argument_errors_are_raised_before_any_device_work():
    from largesteps import distance
    v, f = sx.hand_case("crossing")[:2]
    for fn in (distance.self_intersections, distance.count_self_intersections, distance.fast_find_self_intersections):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 2)), f)
        with pytest.raises(ValueError):
            fn(v, np.zeros((2, 4), np.int64))
        with pytest.raises(TypeError):
            fn(v, f.astype(np.float64))
        with pytest.raises(TypeError):
            fn(v.astype(np.complex64), f)
        with pytest.raises(ValueError, match="no faces"):
            fn(v, np.zeros((0, 3), np.int64))


def test_cpu_tensors_raise():
    from largesteps import distance
    v, f = (torch.from_numpy(x) for x in sx.hand_case("crossing")[:2])
    for fn in (distance.self_intersections, distance.count_self_intersections, distance.fast_find_self_intersections):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(v, f)


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_mesh_selfx_count", "ls_mesh_selfx_pairs", "ls_mesh_selfx_workspace_bytes"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert getattr(native.lib(), name).restype is ctypes.c_int
    assert sorted(n for n in native.EXPORTED_SYMBOLS if n.startswith("ls_mesh_selfx_")) == NAMES
    assert native.lib().ls_version() == 110


def test_abi_argument_checks(native):
    lib = native.lib()
    E, OV = native.LS_E_INVALID, native.LS_E_OVERFLOW
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p(1)                  # never dereferenced: every call below fails an argument check first, or has nothing to do
    n = ctypes.c_size_t(0)
    assert lib.ls_mesh_selfx_count(None, x, x, None, None) == E
    assert lib.ls_mesh_selfx_count(h, None, x, None, None) == E
    assert lib.ls_mesh_selfx_count(h, x, None, x, None) == E
    assert lib.ls_mesh_selfx_workspace_bytes(4, 1, None) == E
    assert lib.ls_mesh_selfx_workspace_bytes(0, 1, ctypes.byref(n)) == E
    assert lib.ls_mesh_selfx_workspace_bytes(4, -1, ctypes.byref(n)) == E
    assert lib.ls_mesh_selfx_workspace_bytes(2 ** 31, 1, ctypes.byref(n)) == OV
    assert lib.ls_mesh_selfx_workspace_bytes(4, 2 ** 30, ctypes.byref(n)) == OV
    assert lib.ls_mesh_selfx_workspace_bytes(4, 0, ctypes.byref(n)) == 0 and n.value >= 4 * 5
    assert lib.ls_mesh_selfx_workspace_bytes(1000, 5000, ctypes.byref(n)) == 0 and n.value >= 4 * 1001 + 4 * 4 * 5000
    assert lib.ls_mesh_selfx_pairs(None, x, 1, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_selfx_pairs(h, None, 1, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_selfx_pairs(h, x, 1, None, x, 1 << 20, None) == E
    assert lib.ls_mesh_selfx_pairs(h, x, 1, x, None, 1 << 20, None) == E
    assert lib.ls_mesh_selfx_pairs(h, x, -1, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_selfx_pairs(h, x, 2 ** 30, x, x, 1 << 20, None) == OV
    assert lib.ls_mesh_selfx_pairs(h, None, 0, None, None, 0, None) == 0                       # k = 0 is a no-op
