"""
tests/lbvh_statement.py without a device: the top-down statement of the hierarchy against a literal transcription of Karras' per-node
searches (k_lbvh_karras of csrc/lbvh.h: direction, the doubling of lmax, the binary search for the other end, the split search, with
delta as in lbvh_delta), `check_invariants` on valid and on deliberately broken arrays, the case table (the cases are conditions on
the codes, asserted here so that they cannot drift), what three ways of breaking the transcription or the sort do to these tests, and the
conditions the references of tests/test_lbvh_gpu.py must meet.
"""
import time

import numpy as np
import pytest

import lbvh_statement as lb
import ray_statement as rs
import selfx_statement as sx

F32 = np.float32
_built = {}


def built(name):
    """(V, F, the statement's arrays) of a case, once; no test writes to them"""
    if name not in _built:
        v, f = lb.case(name)
        _built[name] = (v, f, lb.build(v, f))
    return _built[name]


# ---- Karras, per node --------------------------------------------------------------------------------------------------------------
def clz32(x):
    return 32 - int(x).bit_length()


def karras(k, tie=None, gamma_min=True):
    """(left, right) of k_lbvh_karras over the sorted codes k. `tie` and `gamma_min` break it on purpose: tie = a constant in place of
    32 + clz(i ^ j) for equal codes, gamma_min = False drops the min(d, 0) of the split position"""
    k = [int(x) for x in k]
    T = len(k)

    def delta(i, j):
        if j < 0 or j >= T:
            return -1
        a, b = k[i], k[j]
        if a == b:
            return 32 + clz32(i ^ j) if tie is None else tie
        return clz32(a ^ b)

    left, right = np.zeros(max(T - 1, 0), np.int32), np.zeros(max(T - 1, 0), np.int32)
    for i in range(T - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + (min(d, 0) if gamma_min else 0)
        left[i] = T - 1 + gamma if min(i, j) == gamma else gamma
        right[i] = T - 1 + gamma + 1 if max(i, j) == gamma + 1 else gamma + 1
    return left, right


@pytest.mark.parametrize("name", lb.CASES + ["nan"])
def test_the_statement_is_karras_hierarchy(name):
    v, f, a = built(name)
    left, right = karras(a["code"][a["tri"]])
    assert np.array_equal(left, a["left"]) and np.array_equal(right, a["right"])


@pytest.mark.parametrize("name", lb.CASES + ["nan"])
def test_the_invariants_hold_on_every_statement_tree(name):
    v, f, a = built(name)
    lb.check_invariants(a)
    T = f.shape[0]
    assert a["left"].dtype == np.int32 and a["esc"].shape == (2 * T - 1,) and a["box"].shape == (2 * T - 1, 6) and a["box"].dtype == F32
    assert a["parent"][0] == -1 and a["esc"][0] == -1
    if T > 1:
        assert np.array_equal(a["parent"][a["left"]], np.arange(T - 1)) and np.array_equal(a["parent"][a["right"]], np.arange(T - 1))
    assert not lb.has_negative_zero(v)                       # rule 6: nothing here depends on how fmin orders +0 and -0


def test_the_statement_stays_under_a_second_at_twenty_thousand_faces():
    v, f = lb.case("ico32_far")
    t = time.perf_counter()
    a = lb.build(v, f)
    dt = time.perf_counter() - t
    print(f"build of {f.shape[0]} faces: {dt:.3f} s")
    assert f.shape[0] == 20480 and dt < 1.0
    _built.setdefault("ico32_far", (v, f, a))


# ---- check_invariants notices -------------------------------------------------------------------------------------------------------
def corrupt(a, what):
    a = {k: np.array(x) for k, x in a.items()}
    T = len(a["tri"])
    if what == "left":                                       # two entries swapped: still one parent each, the ranges no longer nest
        a["left"][[3, 200]] = a["left"][[200, 3]]
    elif what == "esc":                                      # one link redirected to another node
        a["esc"][T - 1 + 17] = a["esc"][T - 1 + 18]
    elif what == "box":                                      # one component of an internal box shrunk by an ulp
        a["box"][5, 3] = np.nextafter(a["box"][5, 3], F32(-np.inf))
    elif what == "tri":                                      # two entries made equal
        a["tri"][10] = a["tri"][11]
    return a


@pytest.mark.parametrize("what,named", [("left", "contiguous"), ("esc", "pre-order"), ("box", "box"), ("tri", "tri")])
@pytest.mark.parametrize("name", ["far4096", "far320", "first257"])
def test_the_invariants_name_a_deliberate_corruption(name, what, named):
    a = built(name)[2]
    bad = corrupt(a, what)
    assert lb.differing(a, bad) == [what]
    with pytest.raises(AssertionError, match="^" + named):
        lb.check_invariants(bad)


def test_the_invariants_name_a_node_with_two_parents_and_an_escape_past_a_leaf():
    a = built("far320")[2]
    bad = {k: np.array(x) for k, x in a.items()}
    bad["right"][7] = bad["left"][7]
    with pytest.raises(AssertionError, match="^parent"):
        lb.check_invariants(bad)
    T = len(a["tri"])
    bad = {k: np.array(x) for k, x in a.items()}
    leaf = int(np.nonzero(a["esc"][T - 1:2 * T - 2] < T - 1)[0][0])       # a leaf whose link goes to an internal node: send it a leaf further
    bad["esc"][T - 1 + leaf] = T - 1 + leaf + 2
    with pytest.raises(AssertionError, match="^pre-order"):
        lb.check_invariants(bad)


# ---- the case table is what it claims to be ----------------------------------------------------------------------------------------------
def test_the_far_vertex_cases_collide_as_stated():
    v, f, a = built("far4096")
    assert f.shape[0] == 720 and v.shape[0] == 363 and lb.runs(a["code"]).tolist() == [720]
    assert np.array_equal(a["tri"], np.arange(720))                       # one run: the stable sort keeps the face order
    v, f, a = built("far320")
    r = lb.runs(a["code"])
    assert f.shape[0] == 720 and (r == 1).any() and ((r >= 2) & (r <= 7)).any() and (r >= 8).any()
    print(f"far320: {len(r)} distinct codes, {(r == 1).sum()} runs of 1, {((r >= 2) & (r <= 7)).sum()} of 2-7, {(r >= 8).sum()} of >= 8 (max {r.max()})")
    v, f, a = built("far_face")
    assert f.shape[0] == 721 and (f[-1] == [0, 1, v.shape[0] - 1]).all() and sorted(lb.runs(a["code"]).tolist()) == [1, 720]
    assert a["tri"][-1] == 720                                            # the far face alone in the last cell
    v, f, a = built("repeated")
    assert f.shape[0] == 300 and (f == f[0]).all() and lb.runs(a["code"]).tolist() == [300]


def test_the_icosphere_codes_of_the_existing_suites_are_all_distinct():
    """why these cases are needed: the meshes of the query tests never collide"""
    from largesteps import synthetic
    v, f = lb.sphere()
    assert len(lb.runs(lb.codes(v, f))) == 720
    pv, pf = synthetic.plane(24)
    assert len(lb.runs(lb.codes(pv, pf))) == 1058


@pytest.mark.parametrize("T", lb.SMALL_T)
def test_the_small_trees_have_distinct_codes(T):
    v, f, a = built(f"first{T}")
    assert f.shape[0] == T and (lb.runs(a["code"]) == 1).all() and len(lb.runs(a["code"])) == T
    assert a["left"].shape == (T - 1,) and a["esc"].shape == (2 * T - 1,)


def test_the_flat_plane_takes_the_unit_extent_path():
    v, f, a = built("plane")
    lo, hi = lb.vertex_box(v)
    assert f.shape[0] == 1058 and hi[2] - lo[2] == 0 and (hi[:2] - lo[:2] > 0).all()
    assert (lb.runs(a["code"]) == 1).all() and not (a["code"] & 0x09249249).any()          # the z bits of every code are 0


def test_the_powers_of_two_share_the_first_cell_and_make_a_deep_tree():
    v, f, a = built("powers")
    r = lb.runs(a["code"])
    assert f.shape[0] == 40 and len(r) == 12 and r.max() == 29 and r[0] == 29 and lb.depth(a) == 16
    lo, hi = lb.vertex_box(v)
    assert (lo == 0).all() and (hi == 1).all()
    assert not np.array_equal(a["tri"], np.arange(40))                    # the faces are not given in code order


def test_the_large_case_has_single_and_long_runs():
    v, f, a = built("ico32_far")
    r = lb.runs(a["code"])
    print(f"ico32_far: {len(r)} distinct codes, {(r == 1).sum()} runs of 1, {(r >= 8).sum()} of >= 8 (max {r.max()})")
    assert f.shape[0] == 20480 and (r == 1).any() and (r >= 8).any()


def test_a_nan_coordinate_is_passed_over_by_the_box_and_lands_in_cell_zero():
    v, f, a = built("nan")
    clean = lb.sphere()[0]
    bad = np.nonzero(np.isnan(v).any(1))[0]
    assert bad.size == 1 and np.isnan(v).sum() == 1 and np.isnan(v[bad[0], 0])
    around = np.nonzero((f == bad[0]).any(1))[0]
    assert 5 <= around.size <= 6
    lo, hi = lb.vertex_box(v)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    assert np.array_equal(lo, clean.min(0)) and np.array_equal(hi, clean.max(0))          # the vertex was no extreme of the sphere
    # the x bits of the faces around it are 0, every other code is the clean sphere's
    assert not (a["code"][around] & (0x09249249 << 2)).any()
    rest = np.setdiff1d(np.arange(720), around)
    assert np.array_equal(a["code"][rest], lb.codes(clean, f)[rest])
    assert np.isfinite(a["box"]).all()                       # a face has one NaN corner at the most, and fmin / fmax pass it over
    # an axis that is all NaN: a NaN box, extent 1, cell 0
    w = clean.copy()
    w[:, 1] = np.nan
    assert np.isnan(lb.vertex_box(w)[0][1]) and not (lb.codes(w, f) & (0x09249249 << 1)).any()
    # non-finite centroids of either sign stay inside [0, 1023]
    w = lb.with_far_vertex(clean, np.inf)
    c = lb.codes(w, np.concatenate([f, [[0, 1, 362]]]))
    assert ((c >= 0) & (c < 2 ** 30)).all()


def test_the_slack_of_a_mesh_with_a_nan_is_the_largest_number():
    """the rule of DESIGN.md section 2.12: 2^-40 x the largest |coordinate| that is not a NaN"""
    v = built("nan")[0]
    clean = lb.sphere()[0]
    assert sx.slack(v) == sx.slack(clean) == 2.0 ** -40 * float(np.abs(clean).max())
    w = clean.copy()
    w[np.abs(clean).argmax() // 3, np.abs(clean).argmax() % 3] = np.nan
    assert 0 < sx.slack(w) <= sx.slack(clean)
    assert sx.slack(F32([[np.nan, np.nan, np.nan]])) == 0.0
    assert sx.slack(F32([[-3.0, np.nan, 1.0]])) == 2.0 ** -40 * 3.0


# ---- each of these breaks a named test ---------------------------------------------------------------------------------------------------
COLLIDING = ["far4096", "far320", "far_face", "repeated", "powers", "ico32_far"]


def test_a_constant_tie_break_is_noticed_on_every_colliding_case():
    """32 + clz(i ^ j) replaced by 32: test_the_statement_is_karras_hierarchy fails on each colliding case, and passes on the others"""
    for name in lb.CASES:
        a = built(name)[2]
        left, right = karras(a["code"][a["tri"]], tie=32)
        same = np.array_equal(left, a["left"]) and np.array_equal(right, a["right"])
        assert same == (name not in COLLIDING), name


def test_a_split_without_min_d_0_is_noticed_wherever_a_node_looks_left():
    """gamma = i + s d in place of i + s d + min(d, 0): a node whose range ends at it (d = -1: an internal left child) gets the wrong
    split, and test_the_statement_is_karras_hierarchy fails on every case that has one -- all but the trees of one to three leaves"""
    for name in lb.CASES:
        a = built(name)[2]
        T = len(a["tri"])
        looks_left = bool((a["left"] < T - 1).any())
        assert looks_left == (T > 3), name
        left, right = karras(a["code"][a["tri"]], gamma_min=False)
        same = np.array_equal(left, a["left"]) and np.array_equal(right, a["right"])
        assert same == (not looks_left), name
        if looks_left:
            with pytest.raises(AssertionError):
                lb.check_invariants(dict(a, left=left, right=right))


def test_an_unstable_sort_is_noticed_wherever_codes_collide():
    """equal codes in descending face order: `tri` differs from the statement's on every colliding case, which is what the device's
    arrays are compared with"""
    for name in lb.CASES:
        a = built(name)[2]
        T = len(a["tri"])
        unstable = np.lexsort((-np.arange(T), a["code"])).astype(np.int32)
        assert np.array_equal(a["code"][unstable], a["code"][a["tri"]])                     # still sorted
        assert np.array_equal(unstable, a["tri"]) == (name not in COLLIDING), name


# ---- conditions on the references of the device tests --------------------------------------------------------------------------------------
def test_the_rays_of_the_device_tests_hit_between_a_fifth_and_all():
    """the guard of test_raycast_gpu.check_against_statement on the rays test_lbvh_gpu.py sends: generated from the referenced vertices,
    so that the far vertex does not blow up the box they are aimed at"""
    import torch
    from test_lbvh_gpu import ANSWER_CASES, ray_case
    for name in ANSWER_CASES + ["nan"]:
        v, f, O, D, tr, want = ray_case(name, torch.device("cpu"))
        t, I, W = rs.closest(O, D, v, f, tr)
        assert np.array_equal(t.view(np.int64), want[0].view(np.int64)) and np.array_equal(I, want[1])
        hits = int((I >= 0).sum())
        print(f"{name}: {hits} of {O.shape[0]} rays hit")
        assert 0.2 * O.shape[0] < hits < O.shape[0]
        if name == "repeated":
            assert (I[I >= 0] == 0).all()
        if name == "nan":
            bad = int(np.nonzero(np.isnan(v).any(1))[0][0])
            assert not np.isin(I, np.nonzero((f == bad).any(1))[0]).any()


def test_the_self_intersection_cases_have_pairs():
    from test_lbvh_gpu import selfx_case
    for name in ("jittered_far4096", "jittered_far320", "nan_jittered"):
        v, f, IF = selfx_case(name)
        assert IF.shape[0] > 0, name
    v, f, IF = selfx_case("repeated")
    assert IF.shape[0] == 0
    # the far vertex changes e of the box clause, not the pairs of this mesh
    assert np.array_equal(selfx_case("jittered_far4096")[2], sx.pairs(*sx.jittered(4, 1.0)))
    v, f, IF = selfx_case("nan_jittered")
    bad = int(np.nonzero(np.isnan(v).any(1))[0][0])
    around = np.nonzero((f == bad).any(1))[0]
    # every edge function against a face with a NaN corner has one, and so has an edge that ends at the vertex: such a face is in no pair
    assert not np.isin(IF, around).any() and np.isin(sx.pairs(*sx.jittered(4, 1.0)), around).any()
