"""
The cases of tests/distance_grad_cases.py and the order-exact statement of tests/distance_grad_statement.py, without a device: every
case reaches the branch it was built for (counted from its own arrays); `ordered_gradients`, the fp32 sums in the device's order, agrees
with the fp64 `gradients` within the bound of the device test; and the bitwise comparison of the device test can fail: another point
order inside the faces, or another order of the butterfly, changes bits.
"""
import numpy as np
import pytest

import distance_grad_cases as dc
import distance_grad_statement as dg
import primitives_statement as ps
import remesh_statement as rs


def corner_order(f, nV):
    """(vptr, rank -> corner): the corners grouped by vertex in ascending corner id, the rule of ls_corner_ranks
    (primitives_statement.corner_ranks gives corner -> rank, its inverse)"""
    vptr, cpos = ps.corner_ranks(f, nV)
    order = np.argsort(np.asarray(f).ravel(), kind="stable")
    assert np.array_equal(cpos[order], np.arange(order.size))
    return vptr, order


def walked_on_the_host():
    """(v, f, P, I, C, g) of walked_three_pass with a stand-in for the device's query: a face around the nearest vertex and the closest
    point on it. The two statements are compared on the same (P, I, C, g), whichever face that is"""
    from scipy.spatial import cKDTree
    v, f, p = dc.walked_three_pass()
    v64 = v.astype(np.float64)
    first_face = np.zeros(v.shape[0], dtype=np.int64)
    first_face[f[::-1].ravel()] = np.repeat(np.arange(f.shape[0])[::-1], 3)
    I = first_face[cKDTree(v64).query(p.astype(np.float64))[1]]
    C = rs.point_triangle(p.astype(np.float64), *(v64[f[I, k]] for k in range(3)))
    return v, f, p, I, C, np.random.default_rng(58).uniform(-1.0, 2.0, p.shape[0])


def small_case(name):
    return walked_on_the_host() if name == "walked_three_pass" else dc.fabricated(name)


def test_pass_counts_and_sort_workgroups():
    assert [dc.radix_passes(T) for T in (1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 4]
    v, f, p = dc.walked_three_pass()
    assert f.shape == (67280, 3) and v.shape == (33642, 3) and dc.radix_passes(f.shape[0]) == 3
    assert p.shape[0] >= 33642 + 6 * 64 and dc.rs_chunk(p.shape[0]) == 1024 and dc.sort_workgroups(p.shape[0]) >= 33
    want = {"one_pass_many_blocks": (180, 1), "thresholds": (720, 2), "hub": (dc.HUB_FACES, 2), "out_of_range": (720, 2)}
    for name, (T, passes) in want.items():
        f, I = dc.fabricated_mesh(name)[1], dc.fabricated_ids(name)
        assert f.shape[0] == T and dc.radix_passes(T) == passes, name
        assert dc.rs_chunk(len(I)) == 1024 and dc.sort_workgroups(len(I)) > 1, name
    assert len(dc.fabricated_ids("one_pass_many_blocks")) == 5000
    # one, two and three passes: the order ends in the caller's buffer (odd) and in the scratch's (even), each over several workgroups
    assert {dc.radix_passes(dc.fabricated_mesh(n)[1].shape[0]) for n in dc.FABRICATED} == {1, 2, 3}


def test_the_chunk_cases_sit_on_both_sides_of_both_switches():
    assert [dc.CHUNK_N[n] for n in ("chunk_1024_last", "chunk_2048_first", "chunk_4096_first")] == [2 * 2 ** 20, 2 * 2 ** 20 + 1, 4 * 2 ** 20 + 1]
    assert [dc.rs_chunk(n) for n in (1, 2 * 2 ** 20, 2 * 2 ** 20 + 1, 4 * 2 ** 20, 4 * 2 ** 20 + 1)] == [1024, 1024, 2048, 2048, 4096]
    assert [dc.sort_workgroups(dc.CHUNK_N[n]) for n in ("chunk_1024_last", "chunk_2048_first", "chunk_4096_first")] == [2048, 1025, 1025]
    T = dc.fabricated_mesh("chunk_4096_first")[1].shape[0]
    assert T == 67280 and dc.radix_passes(T) == 3
    for name, n in dc.CHUNK_N.items():
        I = dc.fabricated_ids(name)
        m = np.bincount(I, minlength=T)
        assert len(I) == n and I.min() >= 0 and I.max() < T and len(m) == T
        if n > 4 << 20:                     # about 62 points a face: both paths of the face sum
            assert (m <= 64).sum() > 1000 and (m > 64).sum() > 1000 and (m == 64).any() and (m == 65).any()


def test_thresholds_has_exactly_its_counts_where_it_says():
    v, f = dc.fabricated_mesh("thresholds")
    T = f.shape[0]
    I = dc.fabricated_ids("thresholds")
    m = np.bincount(I, minlength=T)
    assert T == 720 and T % 256 == 208 and T % 64 == 16
    assert np.array_equal(m, dc.threshold_counts()) and set(m.tolist()) == set(dc.THRESHOLD_COUNTS)
    lng = np.nonzero(m > 64)[0]
    assert lng.tolist() == sorted(dc.THRESHOLD_LONG)
    lanes, waves = lng % 64, lng // 64
    assert (lanes == 0).sum() >= 2 and (lanes == 63).sum() >= 2                      # long faces at a wave's first and last lane
    run = [a for a in lng if a + 1 in lng and a + 2 in lng]
    assert run and all(a // 64 == (a + 2) // 64 for a in run)                        # three in a row inside one wave
    assert np.bincount(waves).max() >= 4                                             # the ballot loop takes several turns
    last_wave = lng[lng >= T - 16]
    assert T - 1 in last_wave and len(last_wave) == 2 and waves[-1] == (T - 1) // 64   # two in the partly filled wave, one at T - 1
    for w in set(waves.tolist()):           # empty and short faces in every wave that has a long one
        mw = m[64 * w:64 * w + 64]
        assert (mw == 0).any() and ((mw >= 1) & (mw <= 64)).any(), w
    assert any(m[a + 1] == 0 or m[a - 1] == 0 for a in lng[1:-1]) and any(m[a - 1] == 64 for a in lng[1:])     # and right next to one
    touched = np.zeros(v.shape[0], dtype=bool)
    touched[f[I].ravel()] = True
    assert (~touched).sum() == dc.THRESHOLD_BARE                                       # vertices whose faces hold no point
    # the points of a face are spread through the array
    for a in np.nonzero(m >= 2)[0]:
        at = np.nonzero(I == a)[0]
        assert np.diff(at).max() > 1 and at[-1] - at[0] >= m[a] + 8, a


def test_the_hub_and_the_out_of_range_ids():
    v, f = dc.fabricated_mesh("hub")
    I = dc.fabricated_ids("hub")
    corners = np.bincount(f.ravel(), minlength=v.shape[0])
    assert corners[dc.HUB_VERTEX] == dc.HUB_FACES >= 1000 and np.delete(corners, dc.HUB_VERTEX).max() == 2
    assert all((f[:, k] == dc.HUB_VERTEX).sum() >= 399 for k in range(3))            # the hub at every corner position
    m = np.bincount(I, minlength=f.shape[0])
    assert m.min() >= 1 and (m > 64).sum() == len(dc.HUB_LONG) and all(m[a] == c for a, c in dc.HUB_LONG.items())

    T = dc.fabricated_mesh("out_of_range")[1].shape[0]
    I, base = dc.fabricated_ids("out_of_range"), dc.fabricated_ids("thresholds")
    bad = (I < 0) | (I >= T)
    assert 0.005 <= bad.mean() <= 0.015
    assert set(I[bad].tolist()) == {-1, T, T + 1, 2 ** 40} and np.array_equal(I[~bad], base[~bad])
    assert np.array_equal(dg.keys(I, T)[bad], np.full(bad.sum(), T))
    a, b = dc.fabricated("out_of_range"), dc.fabricated("thresholds")
    for x, y in zip(a[2:], b[2:]):
        assert x is a[3] or np.array_equal(x, y)                                     # the same P, C and g


@pytest.mark.parametrize("name", ("walked_three_pass",) + dc.SMALL_FABRICATED)
def test_ordered_gradients_agree_with_the_fp64_sums(name):
    """|ordered - fp64| <= (depth + 16) 2^-24 sum |terms| for every entry: the bound of the device test"""
    v, f, P, I, C, g = small_case(name)
    vptr, order = corner_order(f, v.shape[0])
    got = dg.ordered_gradients(P, v, f, I, C, g, vptr, order)
    ok = (I >= 0) & (I < f.shape[0])
    want = dg.gradients(P[ok], v, f, I[ok], C[ok], g[ok])
    assert got.dtype == np.float32 and got.shape == v.shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want["gV"])
    bound = (want["depth"][:, None] + 16) * 2.0 ** -24 * want["abs"]
    nz = want["abs"] > 0
    print(f"{name}: {len(I)} points, largest error / bound {float((err[nz] / bound[nz]).max()):.3e}, deepest chain {int(want['depth'].max())}")
    assert nz.any() and (err <= bound).all()
    assert not got[~nz].any()


def test_another_order_changes_bits():
    """what the bitwise comparison of the device test rests on: it tells the stated order from its neighbours"""
    v, f, P, I, C, g = dc.fabricated("thresholds")
    vptr, order = corner_order(f, v.shape[0])
    want = dg.ordered_gradients(P, v, f, I, C, g, vptr, order)
    assert np.array_equal(want.view(np.int32), dg.ordered_gradients(P, v, f, I, C, g, vptr, order).view(np.int32))
    # descending point id inside every face: the same points in reverse, so the stable sort hands them over reversed
    back = dg.ordered_gradients(P[::-1], v, f, I[::-1], C[::-1], g[::-1], vptr, order)
    assert (back.view(np.int32) != want.view(np.int32)).any()
    up = dg.ordered_gradients(P, v, f, I, C, g, vptr, order, butterfly=(1, 2, 4, 8, 16, 32))
    assert (up.view(np.int32) != want.view(np.int32)).any()
    # and only the long faces see the butterfly: with every face at 64 points or fewer the two agree
    keep = np.bincount(I, minlength=f.shape[0])[I] <= 64
    a = dg.ordered_gradients(P[keep], v, f, I[keep], C[keep], g[keep], vptr, order)
    b = dg.ordered_gradients(P[keep], v, f, I[keep], C[keep], g[keep], vptr, order, butterfly=(1, 2, 4, 8, 16, 32))
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # the corners of a vertex in descending corner id
    rev = np.concatenate([order[vptr[k]:vptr[k + 1]][::-1] for k in range(v.shape[0])])
    assert (dg.ordered_gradients(P, v, f, I, C, g, vptr, rev).view(np.int32) != want.view(np.int32)).any()
