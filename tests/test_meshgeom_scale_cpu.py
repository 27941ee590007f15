"""
What tests/test_meshgeom_scale_gpu.py stands on, without a GPU: the cases of tests/meshgeom_scale_cases.py cross the thresholds they are
there for (with the constants csrc/ is compiled from), the fp64 sums of the average are exact on them, and the fp32 statement in the
kernels' order (tests/meshgeom_ordered.py) is the same function as the fp64 statement (tests/meshgeom_statement.py).
"""
import math

import numpy as np
import pytest

import meshgeom_ordered as mo
import meshgeom_scale_cases as mc
import meshgeom_statement as ms


def test_the_sources_use_the_constants_as_the_cases_assume():
    for name, lines in mc.USES.items():
        src = mc.nc.source(name)
        for line in lines:
            assert line in src, f"csrc/{name} no longer has `{line}`: the formulas of meshgeom_scale_cases.py stand for it"
    assert mc.SWEEP == mc.MESH_MAXG * mc.BLOCK and mc.BLOCK % mc.WAVE == 0 and mc.BLOCK > mc.WAVE
    assert mc.VG > 1 and mc.GC > 1                           # request groups: there are remainders to cover
    assert len(set(mc.CASES)) == len(mc.CASES) == 22


def test_sweep_cases_cross_the_capped_grid():
    """k_edge_length_partials: G = reduce_grid(F) workgroups, a thread's loop steps by G * BLOCK"""
    S, B = mc.SWEEP, mc.BLOCK
    whole = 2 * (mc.PLANE - 1) ** 2
    assert mc.SWEEP_SIZES == (S - 1, S, S + 1, S + B, S + B + 1, 2 * S, 2 * S + 1, whole)
    facts = {F: (mc.partials(F), mc.trips(F), mc.last_trip(F)) for F in mc.SWEEP_SIZES}
    G = mc.MESH_MAXG
    assert facts[S - 1] == (G, 1, S - 1)                     # the full grid, its last thread without a face
    assert facts[S] == (G, 1, S)                             # every thread one face, nobody loops
    assert facts[S + 1] == (G, 2, 1)                         # one thread loops, for one face
    assert facts[S + B] == (G, 2, B)                         # the first workgroup loops, whole
    assert facts[S + B + 1] == (G, 2, B + 1)                 # ... and one thread of the second
    assert facts[2 * S] == (G, 2, S)                         # every thread two faces
    assert facts[2 * S + 1] == (G, 3, 1)                     # a third trip for one face
    assert facts[whole][:2] == (G, 3) and B < facts[whole][2] < S and facts[whole][2] % B != 0
    F2 = 2 * (mc.PLANE_2 - 1) ** 2
    assert (mc.partials(F2), mc.trips(F2)) == (G, 2) and B < mc.last_trip(F2) < S and 2 * (mc.PLANE_2 - 2) ** 2 <= S
    pv, pf = mc.nc.jittered_plane(mc.PLANE)
    for name, F in zip(mc.SWEEP_CASES, mc.SWEEP_SIZES):
        v, f = mc.mesh(name)
        assert f.shape == (F, 3) and F <= whole and v.shape == pv.shape == (mc.PLANE ** 2, 3)
        assert np.array_equal(f, pf[:F]) and np.array_equal(v, pv)
        assert (mc.valence(name)[-3:] == 0).all() == (F < whole)       # a slice leaves trailing unreferenced vertices
    v, f = mc.mesh(mc.SWEEP_CASES[-1])
    assert f.shape == (F2, 3) and v.shape == (mc.PLANE_2 ** 2, 3)


def test_small_cases_cross_a_wave_and_a_workgroup():
    W, B = mc.WAVE, mc.BLOCK
    assert mc.SMALL_SIZES == (1, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1)
    assert [mc.partials(F) for F in mc.SMALL_SIZES] == [1, 1, 1, 1, 1, 1, 2, 3]        # one partial, two, three ...
    assert all(mc.trips(F) == 1 for F in mc.SMALL_SIZES)
    assert (B + 1) - B == 1 and (2 * B + 1) - 2 * B == 1                               # ... the last workgroup with one face
    for name, F in zip(mc.SMALL_CASES, mc.SMALL_SIZES):
        v, f = mc.mesh(name)
        assert f.shape == (F, 3) and v.shape == (mc.PLANE ** 2, 3) and (mc.valence(name)[-3:] == 0).all()


@pytest.mark.parametrize("name", mc.SWEEP_CASES + mc.SMALL_CASES)
def test_the_average_is_exactly_predictable(name):
    """the perimeters span few binades: every fp64 partial sum is exact (three orders agree), so the kernel's result is one rounding of
    the exact sum -- and one face lost or counted twice changes its bits"""
    v, f = mc.mesh(name)
    per = mo.perimeters(v, f)
    F = per.shape[0]
    assert mo.exact_bits(per) <= 53
    if name == f"sweep{2 * (mc.PLANE - 1) ** 2}":
        assert mo.exact_bits(per) == 46
    if name == f"sweep_plane{mc.PLANE_2}":
        assert mo.exact_bits(per) == 45
    per64 = per.astype(np.float64)
    total = math.fsum(per.tolist())
    assert total == per64.sum() == per64[::-1].cumsum()[-1]
    # strided as the kernel's grid sees them: a partial per workgroup, then the partials
    G = mc.partials(F)
    pad = np.zeros(-(-F // (G * mc.BLOCK)) * G * mc.BLOCK)
    pad[:F] = per64
    assert pad.reshape(-1, G, mc.BLOCK).sum(axis=(0, 2)).sum() == total
    avg = mo.average(v, f)
    assert avg.dtype == np.float32 and avg.shape == ()
    a64 = ms.average_edge_length(v, f, np.float64)
    assert abs(float(avg) - a64) <= 1e-6 * a64
    if F > 1:                                                # (the only face lost leaves 0)
        for lost in (total - per64.min(), total + per64.min()):
            other = np.float32(lost) / np.float32(F) / np.float32(3)
            assert other != avg, "a face lost or counted twice would not change the result's bits"
        if F >= mc.SWEEP:                                    # at least 10 ulp: far from a chance agreement
            assert abs(float(other) - float(avg)) >= 10 * float(np.spacing(avg))


def test_ladder_has_every_clamp_position():
    v, f = mc.mesh("ladder")
    val = mc.valence("ladder")
    assert v.shape == (1150, 3) and f.shape == (1122, 3) and v.dtype == np.float32 and f.dtype == np.int64
    hub = int(val.argmax())
    assert val[hub] == mc.HUB == 4 * mc.BLOCK + 7 > mc.BLOCK
    assert set(val.tolist()) == set(mc.LADDER_FANS) == set(range(1, 14)) | {mc.HUB}
    assert [int((f[:, j] == hub).sum()) for j in range(3)] == [344, 344, 343]          # the hub's corners over the three slots
    for k in mc.LADDER_FANS[2:]:                             # one apex per fan (valences 1 and 2 also belong to rim vertices)
        assert (val == k).sum() == 1
        apex = int(np.nonzero(val == k)[0][0])
        assert set(np.nonzero(f == apex)[1].tolist()) == {0, 1, 2}                     # ... in every corner slot
    for group in (mc.VG, mc.GC):                             # every clamp position of both request groups
        assert {k % group for k in mc.LADDER_FANS} == set(range(group))
    tails = {k - mc.GC for k in mc.LADDER_FANS if k > mc.GC}  # what the tail loop of k_gather_corners is left with
    assert 1 in tails and len(tails) >= 3 and max(tails) > mc.BLOCK
    assert not np.array_equal(np.sort(f[:, 0]), f[:, 0]) and not np.array_equal(np.sort(val)[::-1], val)      # permuted
    mass = ms.massmatrix_voronoi(v, f, np.float32)
    assert mass.dtype == np.float32 and np.isfinite(mass).all() and (mass > 0).all()
    T = ms.face_terms(v, f, np.float32)
    # both branches of the cells: the hub's needles are obtuse at the rim, the wide triangles of the small fans mostly are not
    assert T["obtuse"].any(axis=1).sum() >= 50 and (~T["obtuse"].any(axis=1)).sum() >= 50
    assert np.isfinite(mo.corner_rows_mass(v, f, mc.mass_weights("ladder"), T)).all()


def test_pad_cases_sit_around_one_workgroup_of_vertices():
    B = mc.BLOCK
    assert mc.PAD_SIZES == (B - 1, B, B + 1)
    n = mc.PAD_PLANE
    assert n * n < B - 1
    for name, V in zip(mc.PAD_CASES, mc.PAD_SIZES):
        v, f = mc.mesh(name)
        val = mc.valence(name)
        assert v.shape == (V, 3) and f.shape == (2 * (n - 1) ** 2, 3)
        assert (val[:n * n] > 0).all() and (val[n * n:] == 0).all()
        assert [-(-V // B) for V in mc.PAD_SIZES] == [1, 1, 2]
    v, f = mc.mesh("pad_f128")
    val = mc.valence("pad_f128")
    assert f.shape == (128, 3) and (36 * 128) % 512 == 0     # the corner buffer ends on the allocator's rounding
    assert (val[-3:] == 0).all() and val[-4] > 0 and v.shape[0] == f.max() + 4


SMALLER = mc.SMALL_CASES + ("ladder",) + mc.PAD_CASES + (f"sweep_plane{mc.PLANE_2}",)


@pytest.mark.parametrize("name", SMALLER)
def test_ordered_backwards_are_the_statement(name):
    """the criteria of test_hip_1m_vertices_vs_statement, for the fp32 statement in the kernels' order instead of the kernels"""
    v, f = mc.mesh(name)
    V = v.shape[0]
    T = ms.face_terms(v, f, np.float32)
    w = mc.mass_weights(name)
    obtuse = T["obtuse"]
    kap = ms.vertex_condition(v, f)[:, None]
    g64, mag = ms.massmatrix_voronoi_backward(v, f, w, obtuse=obtuse, magnitude=True)
    g32 = mo.gather(mo.corner_rows_mass(v, f, w, T), f, V)
    assert g32.dtype == np.float32 and np.isfinite(g32).all()
    assert (np.abs(g32 - g64) <= 1e-5 * mag * kap).all()
    for g in mc.AVG_WEIGHTS:
        ga64, mag = ms.average_edge_length_backward(v, f, g, magnitude=True)
        ga32 = mo.gather(mo.corner_rows_avg(v, f, g, T), f, V)
        assert ga32.dtype == np.float32 and (np.abs(ga32 - ga64) <= 1e-6 * mag).all()
        assert not ga32[mc.valence(name) == 0].any() and np.abs(ga32).max() > 0
    a64 = ms.average_edge_length(v, f, np.float64)
    assert abs(float(mo.average(v, f, T)) - a64) <= 1e-6 * a64


def test_gather_is_the_sequential_sum_in_corner_order():
    """against the plainest loop, on the ladder (valences 1 .. 1031, permuted faces)"""
    v, f = mc.mesh("ladder")
    rows = np.random.default_rng(3).standard_normal((f.shape[0], 3, 3)).astype(np.float32)
    want = np.zeros((v.shape[0], 3), np.float32)
    for c in range(3 * f.shape[0]):                          # ascending corner id 3 f + i
        want[f[c // 3, c % 3]] += rows[c // 3, c % 3]
    got = mo.gather(rows, f, v.shape[0])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
