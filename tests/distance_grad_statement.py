"""
Statement of the gradient of the point-to-mesh squared distance (csrc/distance.hip, largesteps.distance): the
barycentric weights of the closest point and the two gradients, in numpy fp64, with the operations of the device code in its order
(the build has -ffp-contract=off, so the weights come out with the same bits).

1. Weights. For a point p and its face (a, b, c) the closest point is C = w_a a + w_b b + w_c c, and w follows the region tests of
   remesh_statement.point_triangle: vertex regions (1,0,0), (0,1,0), (0,0,1); edge ab with v = d1 / (d1 - d3): (1 - v, v, 0); edge ac with
   w = d2 / (d2 - d6): (1 - w, 0, w); edge bc with w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (0, 1 - w, w); interior with
   den = 1 / ((va + vb) + vc), v = vb den, w = vc den: ((1 - v) - w, v, w). A degenerate face (distance_statement rule 2) takes the segment
   that rule picks (ab, bc, ca; a later one only when strictly closer): with t = ap . ab and l = ab . ab its ends get (1, 0) when t <= 0,
   (0, 1) when t >= l, else (1 - t / l, t / l); the third corner gets 0.
2. Gradient. With d = p - C (fp64, C as the query returned it) and g the incoming gradient of sqrD: the term of point i to p_i is
   fl32((2 g) d), its term to corner k of its face fl32(-((2 g) w_k) d): formed in fp64, rounded to fp32 once. The gradient to a vertex
   is the sum of the terms of the corners that are this vertex (a repeated index receives both of its terms).
The device adds the terms in fp32 in a fixed order; `gradients` adds them in fp64 and reports, per vertex, the sum of their magnitudes
and the length of the device's fp32 chain, which is what the error bound of the device test is made of.
3. Order. `ordered_gradients` adds them in fp32 in the device's order, so its result is the device's bit for bit. The key of a point is
   its face, or F (the number of faces, "no group") for an I outside [0, F); the points are sorted stably by key, so a face's points
   come in ascending point id, and those of key F are dropped. The nine-entry row of a face with m points starts from +0.0f; up to
   m = 64 it is one chain over items 0, 1, ..., m - 1; a longer one is 64 lane chains, lane l over items l, l + 64, ..., then
   v = v + v[lane ^ s] for s = 32, 16, 8, 4, 2, 1, and lane 0 is the row. A vertex adds, from +0.0f, the three entries of its corners
   in rank order: corner c is entries 3 (c % 3) ... + 2 of row c // 3.
"""
import numpy as np

import distance_statement as ds
import remesh_statement as rs


def tri_weights(p, a, b, c):
    """rule 1 on a non-degenerate face, broadcast over leading axes: (..., 3)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = rs._d(ab, ap), rs._d(ac, ap)
        bp = p - b
        d3, d4 = rs._d(ab, bp), rs._d(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = rs._d(ab, cp), rs._d(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        zero, one = np.zeros_like(v), np.ones_like(v)
        out = np.stack([(1.0 - v) - w, v, w], -1)
        for cond, val in ((((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)), (zero, 1.0 - w_bc, w_bc)),
                          (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), (1.0 - w_ac, zero, w_ac)),
                          (((d6 >= 0) & (d5 <= d6)), (zero, zero, one)),
                          (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), (1.0 - v_ab, v_ab, zero)),
                          (((d3 >= 0) & (d4 <= d3)), (zero, one, zero)),
                          (((d1 <= 0) & (d2 <= 0)), (one, zero, zero))):
            out = np.where(cond[..., None], np.stack(val, -1), out)
    return out


def seg_weights(p, a, b):
    """the weights of distance_statement.point_segment's point on the ends a, b"""
    ab = b - a
    t, l = rs._d(p - a, ab), rs._d(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = t / l
    wa, wb = 1.0 - s, s
    wa, wb = np.where(t >= l, 0.0, wa), np.where(t >= l, 1.0, wb)
    return np.where(t <= 0, 1.0, wa), np.where(t <= 0, 0.0, wb)


def segment_weights_of_face(p, a, b, c):
    zero = np.zeros(np.broadcast(p[..., 0], a[..., 0]).shape)
    d = ds.sq(p, ds.point_segment(p, a, b))
    u0, u1 = seg_weights(p, a, b)
    w = np.stack([u0 + zero, u1 + zero, zero], -1)
    e = ds.sq(p, ds.point_segment(p, b, c))
    u0, u1 = seg_weights(p, b, c)
    closer = e < d
    w = np.where(closer[..., None], np.stack([zero, u0 + zero, u1 + zero], -1), w)
    d = np.where(closer, e, d)
    e = ds.sq(p, ds.point_segment(p, c, a))
    u0, u1 = seg_weights(p, c, a)
    return np.where((e < d)[..., None], np.stack([u1 + zero, zero, u0 + zero], -1), w)


def face_weights(p, a, b, c):
    """rule 1 with the guard of distance_statement.point_face"""
    r = rs.point_triangle(p, a, b, c)
    ok = (ds.area_term(a, b, c) > 0) & np.isfinite(r).all(-1)
    w = tri_weights(p, a, b, c)
    if ok.all():
        return w
    return np.where(ok[..., None], w, segment_weights_of_face(p, a, b, c))


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def weights(P, V, F, I):
    """(n, 3) fp64: the weights of point P[i] on face F[I[i]]"""
    P, V, F = _f64(P), _f64(V), np.asarray(F, dtype=np.int64)
    if P.shape[0] == 0:
        return np.zeros((0, 3))
    a, b, c = (V[F[I, k]] for k in range(3))
    return face_weights(P, a, b, c)


def terms(P, V, F, I, C, g):
    """rule 2 before the rounding: (tP (n, 3), tV (n, 3 corners, 3)) fp64"""
    P = _f64(P)
    d = P - np.asarray(C, dtype=np.float64)
    s = 2.0 * np.asarray(g, dtype=np.float64)
    w = weights(P, V, F, I)
    tP = s[:, None] * d
    tV = -((s[:, None] * w)[:, :, None] * d[:, None, :])
    return tP, tV


def chain(m):
    """the fp32 additions of a face's row of m points: one thread in order up to 64, else lane-strided and the butterfly"""
    m = np.asarray(m)
    return np.where(m <= 64, m, -(-m // 64) + 6)


def gradients(P, V, F, I, C, g, t=None):
    """dict: gP (n, 3) fp32; gV (nV, 3) fp64, the exact sum of the fp32 terms; abs (nV, 3) the sum of their magnitudes; depth (nV,) the
    device's fp32 chain: the longest row chain among the vertex's faces plus the number of its corners. t: terms(P, V, F, I, C, g) of a
    caller that has them already"""
    F = np.asarray(F, dtype=np.int64)
    I = np.asarray(I, dtype=np.int64)
    nV, nF = np.asarray(V).shape[0], F.shape[0]
    tP, tV = terms(P, V, F, I, C, g) if t is None else t
    tV = tV.astype(np.float32).astype(np.float64)
    gV, ab = np.zeros((nV, 3)), np.zeros((nV, 3))
    for k in range(3):
        np.add.at(gV, F[I, k], tV[:, k])
        np.add.at(ab, F[I, k], np.abs(tV[:, k]))
    per_face = chain(np.bincount(I, minlength=nF))
    longest = np.zeros(nV, dtype=np.int64)
    np.maximum.at(longest, F.reshape(-1), np.repeat(per_face, 3))
    corners = np.bincount(F.reshape(-1), minlength=nV)
    return {"gP": tP.astype(np.float32), "gV": gV, "abs": ab, "depth": longest + corners}


def point_terms(P, C, g):
    """rule 2 to the points alone, (n, 3) fp32: it needs no face, so a point whose I is outside [0, F) has its term too"""
    return ((2.0 * np.asarray(g, dtype=np.float64))[:, None] * (_f64(P) - np.asarray(C, dtype=np.float64))).astype(np.float32)


BUTTERFLY = (32, 16, 8, 4, 2, 1)


def keys(I, nF):
    """rule 3: the face of a point, or nF for an I outside [0, nF)"""
    I = np.asarray(I, dtype=np.int64)
    return np.where((I < 0) | (I >= nF), nF, I)


def face_rows(t, key, nF, butterfly=BUTTERFLY):
    """rule 3 up to the rows: t (n, 9) fp32, the terms of every point; key (n,) in [0, nF] -> (nF, 9) fp32. Vectorised over the faces,
    looping over the position in the chain"""
    t, key = np.asarray(t, dtype=np.float32), np.asarray(key, dtype=np.int64)
    order = np.argsort(key, kind="stable")
    order = order[key[order] < nF]
    m = np.bincount(key[order], minlength=nF)
    seg = np.r_[0, np.cumsum(m)]
    t = t[order]
    rows = np.zeros((nF, 9), dtype=np.float32)
    short = m <= 64
    for j in range(int(m[short].max(initial=0))):
        a = np.nonzero(short & (m > j))[0]
        rows[a] += t[seg[a] + j]
    lng = np.nonzero(~short)[0]
    if lng.size:
        lanes = np.arange(64)
        acc = np.zeros((lng.size, 64, 9), dtype=np.float32)
        for r in range(-(-int(m[lng].max()) // 64)):
            item = 64 * r + lanes
            a, l = np.nonzero(item[None, :] < m[lng][:, None])
            acc[a, l] += t[seg[lng[a]] + item[l]]
        for s in butterfly:
            acc = acc + acc[:, lanes ^ s]
        rows[lng] = acc[:, 0]
    return rows


def vertex_sums(rows, vptr, corner_order):
    """rule 3 from the rows on: (nV, 3) fp32, vectorised over the vertices, looping over the rank"""
    vptr, corner_order = np.asarray(vptr, dtype=np.int64), np.asarray(corner_order, dtype=np.int64)
    of_corner = rows.reshape(-1, 3)                  # corner c: entries 3 (c % 3) ... + 2 of row c // 3
    cnt = np.diff(vptr)
    gV = np.zeros((cnt.size, 3), dtype=np.float32)
    for j in range(int(cnt.max(initial=0))):
        a = np.nonzero(cnt > j)[0]
        gV[a] += of_corner[corner_order[vptr[a] + j]]
    return gV


def ordered_gradients(P, V, F, I, C, g, vptr, corner_order, butterfly=BUTTERFLY, t=None):
    """(nV, 3) fp32: the gradient to V with the bits of the device (rule 3). vptr (nV + 1,) and corner_order (3 nF,) are the corner
    ranking: the corners of vertex v are corner_order[vptr[v] : vptr[v + 1]]. `butterfly` is there for the test that a different order
    of the lane sums changes bits. t: the terms(...) of the points whose I is in [0, F), in their order, of a caller that has them"""
    F = np.asarray(F, dtype=np.int64)
    key = keys(I, F.shape[0])
    ok = key < F.shape[0]
    if t is None:
        t = terms(np.asarray(P)[ok], V, F, key[ok], np.asarray(C)[ok], np.asarray(g)[ok])
    tV = t[1].astype(np.float32).reshape(-1, 9)
    return vertex_sums(face_rows(tV, key[ok], F.shape[0], butterfly), vptr, corner_order)
