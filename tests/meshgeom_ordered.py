"""
The backwards of csrc/meshgeom.hip and its average in numpy fp32, operation by operation in the KERNELS' association -- what
tests/test_meshgeom_scale_gpu.py compares bits with. tests/meshgeom_statement.py states the same graph, but a sum such as
`gl[k1] += 2.0f * (gden * l[k2]) + 2.0f * gnum * l[k1]` adds the two products first in the kernel and one after the other there: equal in
exact arithmetic, not in fp32. The forward intermediates are ms.face_terms(v, f, np.float32), which already follows voronoi_face.

    corner_rows_avg / corner_rows_mass   (F, 3, 3): the gv of k_edge_length_bwd / voronoi_face_bwd, row i = the face's corner i
    gather                               the per-vertex sum of k_gather_corners: a vertex's corners in rank order (ascending corner id
                                         3 f + i), sequential fp32 from 0
    average                              k_edge_length_partials + k_edge_length_finish: the EXACT sum of the fp32 perimeters (the fp64
                                         partial sums are exact in any order under exact_bits), rounded once, / F / 3 in fp32
"""
import numpy as np

import meshgeom_statement as ms

F32 = np.float32


def _terms(v, f, T):
    T = ms.face_terms(v, f, F32) if T is None else T
    assert T["A"].dtype == F32 and T["p"][0].dtype == F32
    return T


def _rows_from_edges(T, w):
    """the last loop of both backwards: edge k (from corner k2 to corner k1) adds d_k * w_k to corner k1 and subtracts it from corner k2,
    k = 0, 1, 2 in turn onto rows that start at 0"""
    F = T["A"].shape[0]
    gv = np.zeros((F, 3, 3), F32)
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        gd = (T["p"][k1] - T["p"][k2]) * w[k][:, None]
        gv[:, k1] = gv[:, k1] + gd
        gv[:, k2] = gv[:, k2] - gd
    assert gv.dtype == F32
    return gv


def perimeters(v, f, T=None):
    """(F,) fp32: (l0 + l1) + l2, as k_edge_length_partials adds them"""
    T = _terms(v, f, T)
    return (T["l"][0] + T["l"][1]) + T["l"][2]


def exact_bits(per):
    """the bits an exact sum of these fp32 values needs: ceil(log2 F) + exponent span + 25 -- every value is a multiple of
    2^(emin - 23) and the sum of F of them is below 2^(emax + 1 + ceil(log2 F)). At most 53: every fp64 partial sum, in any order, is exact."""
    assert per.dtype == F32 and np.isfinite(per).all() and (per > 0).all()
    e = np.frexp(per)[1]
    return (per.shape[0] - 1).bit_length() + int(e.max() - e.min()) + 25


def average(v, f, T=None):
    """0-dim fp32: float32(exact sum of the perimeters) / float32(F) / float32(3)"""
    per = perimeters(v, f, T)
    assert exact_bits(per) <= 53                             # numpy's fp64 sum is then exact too, whatever its order
    return F32(per.astype(np.float64).sum()) / F32(per.shape[0]) / F32(3)


def corner_rows_avg(v, f, g, T=None):
    """k_edge_length_bwd: c = (g / 3) / F, w_k = c / l_k (0 for a zero-length edge)"""
    T = _terms(v, f, T)
    c = (F32(g) / F32(3)) / F32(np.asarray(f).shape[0])
    with np.errstate(all="ignore"):
        return _rows_from_edges(T, [np.where(lk == 0, F32(0), c / lk) for lk in T["l"]])


def corner_rows_mass(v, f, g_mass, T=None):
    """voronoi_face_bwd with gc = g_mass at the face's three vertices"""
    T = _terms(v, f, T)
    f = np.asarray(f, np.int64)
    g_mass = np.asarray(g_mass)
    assert g_mass.dtype == F32
    l, cs, den, bary, s, S, A, r, obtuse = T["l"], T["cos"], T["den"], T["bary"], T["s"], T["S"], T["A"], T["r"], T["obtuse"]
    G = [g_mass[f[:, j]].copy() for j in range(3)]
    zero = np.zeros_like(A)
    with np.errstate(all="ignore"):
        gA = zero.copy()
        for k in (2, 1, 0):                                  # the overrides, last applied first: only where the corner is obtuse
            m = obtuse[:, k]
            for j in (2, 1, 0):
                gA = np.where(m, gA + F32(0.5 if j == k else 0.25) * G[j], gA)
                G[j] = np.where(m, zero, G[j])
        gl = [zero.copy() for _ in range(3)]
        gbraw, gS = [], zero.copy()
        for k in range(3):
            gt = F32(0.5) * G[(k + 1) % 3] + F32(0.5) * G[(k + 2) % 3]
            gA = gA + gt * bary[k]
            gb = gt * A
            gbraw.append(gb / S)
            gS = gS - gb * (bary[k] / S)
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            gbr = gbraw[k] + gS
            gcos = gbr * l[k]
            gl[k] = gl[k] + gbr * cs[k]
            gnum = gcos / den[k]
            gden = -gcos * (cs[k] / den[k])
            gl[k1] = gl[k1] + (F32(2) * (gden * l[k2]) + (F32(2) * gnum) * l[k1])      # the two products first, then onto gl
            gl[k2] = gl[k2] + (gden * (F32(2) * l[k1]) + (F32(2) * gnum) * l[k2])
            gl[k] = gl[k] - (F32(2) * gnum) * l[k]
        gP = (F32(0.25) * gA) / (F32(2) * r)
        gs3 = gP * ((s[0] * s[1]) * s[2])
        g012 = gP * s[3]
        gs2 = g012 * (s[0] * s[1])
        g01 = g012 * s[2]
        gs0, gs1 = g01 * s[1], g01 * s[0]
        gl[0] = gl[0] + (((gs0 + gs1) + gs2) - gs3)          # `gl[0] += gs0 + gs1 + gs2 - gs3`: the right-hand side first
        gl[1] = gl[1] + (((gs0 + gs1) - gs2) + gs3)
        gl[2] = gl[2] + (((gs0 - gs1) + gs2) + gs3)
        assert all(x.dtype == F32 for x in gl)
        return _rows_from_edges(T, [np.where(l[k] == 0, F32(0), gl[k] / l[k]) for k in range(3)])


def gather(rows, f, V):
    """(V, 3) fp32: x = 0; x += the vertex's corner rows in ascending corner id. One loop over the rank position, all vertices that still
    have a corner at that position at once."""
    f = np.asarray(f, np.int64)
    rows = np.asarray(rows)
    assert rows.dtype == F32 and rows.shape == (f.shape[0], 3, 3)
    flat = rows.reshape(-1, 3)
    owner = f.reshape(-1)
    order = np.argsort(owner, kind="stable")                 # vertex-major, ascending corner id within a vertex: the ranking
    cnt = np.bincount(owner, minlength=V)
    vptr = np.concatenate([[0], np.cumsum(cnt)])
    by_valence = np.argsort(-cnt, kind="stable")             # the vertices with a corner at position r are a prefix of this
    alive = np.searchsorted(-cnt[by_valence], -np.arange(cnt.max(initial=0)), side="left")
    out = np.zeros((V, 3), F32)
    for r in range(cnt.max(initial=0)):
        vs = by_valence[:alive[r]]                           # cnt > r
        out[vs] = out[vs] + flat[order[vptr[vs] + r]]
    return out
