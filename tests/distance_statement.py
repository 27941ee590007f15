"""
Statement of the point-to-mesh distance of csrc/distance.hip (largesteps.distance): a brute force over every (point, face) pair, in
numpy and in torch (fp64, any device). The device's LBVH answers with the same bits.

Rules:
1. Arithmetic is fp64 from the fp32 coordinates of the query points and the mesh.
2. The closest point r of p on face (a, b, c): when the area term A = |ab x ac|^2 (cx = ab_y ac_z - ab_z ac_y, ..., A = (cx cx + cy cy)
   + cz cz) is positive, r is remesh_statement.point_triangle(p, a, b, c) (the remesher's region tests). When A is not positive (a
   repeated index, collinear corners), or when that r is not finite, the face is degenerate: r is the closest of the closest points on
   its segments ab, bc, ca, in that order (a later segment replaces an earlier one only when strictly closer).
3. The closest point on segment (a, b): t = ap . ab, l = ab . ab; a when t <= 0, else b when t >= l, else a + ab (t / l).
4. The squared distance of p to r is (dx dx + dy dy) + dz dz of p - r; the squared distance of p to the mesh is its minimum over the
   faces, and the face I is the lowest id among those that reach it (the tie rule). C is that face's r.
5. hausdorff(VA, FA, VB, FB) = sqrt(max(max_a d2(a, B), max_b d2(b, A))) over every row of VA and VB as query points: libigl's
   definition, vertex-to-surface (not the surfaces' Hausdorff distance, libigl's documented known issue).
No finite input gives a NaN: the region tests can divide by zero only on the faces that rule 2 sends to their segments, and rule 3
divides only by l > t > 0.
"""
import math

import numpy as np

import remesh_statement as rs

F64 = np.float64


# ---- one face ---------------------------------------------------------------------------------------------------------------
def area_term(a, b, c):
    ab, ac = b - a, c - a
    cx = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
    cy = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
    cz = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    return (cx * cx + cy * cy) + cz * cz


def sq(p, r):
    d = p - r
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def point_segment(p, a, b):
    ab = b - a
    t, l = rs._d(p - a, ab), rs._d(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = a + ab * (t / l)[..., None]
    r = np.where((t >= l)[..., None], np.broadcast_to(b, r.shape), r)
    return np.where((t <= 0)[..., None], np.broadcast_to(a, r.shape), r)


def closest_segment(p, a, b, c):
    r = point_segment(p, a, b)
    d = sq(p, r)
    for u, w in ((b, c), (c, a)):
        s = point_segment(p, u, w)
        e = sq(p, s)
        closer = e < d
        r = np.where(closer[..., None], s, r)
        d = np.where(closer, e, d)
    return r


def point_face(p, a, b, c):
    """rule 2: the closest point of p on face (a, b, c), broadcast over leading axes"""
    r = rs.point_triangle(p, a, b, c)
    ok = (area_term(a, b, c) > 0) & np.isfinite(r).all(-1)
    if ok.all():
        return r
    return np.where(ok[..., None], r, closest_segment(p, a, b, c))


# ---- the mesh ---------------------------------------------------------------------------------------------------------------
def squared_distance(P, V, F, chunk=256):
    """(sqrD (n,), I (n,) int64, C (n, 3)) of the points P to the mesh (V, F), fp64 numpy"""
    P = np.asarray(P, dtype=np.float32).astype(F64)
    V = np.asarray(V, dtype=np.float32).astype(F64)
    F = np.asarray(F, dtype=np.int64)
    A, B, C = (V[F[:, k]][None] for k in range(3))
    n = P.shape[0]
    sqrD, I, Cl = np.empty(n), np.empty(n, dtype=np.int64), np.empty((n, 3))
    for s in range(0, n, chunk):
        p = P[s:s + chunk, None, :]
        q = point_face(p, A, B, C)
        d2 = sq(p, q)
        j = np.argmin(d2, axis=1)                    # the first minimum: the lowest face id
        rows = np.arange(j.size)
        sqrD[s:s + chunk], I[s:s + chunk], Cl[s:s + chunk] = d2[rows, j], j, q[rows, j]
    return sqrD, I, Cl


def hausdorff(VA, FA, VB, FB, squared=squared_distance):
    ab = float(np.max(squared(VA, VB, FB)[0]))
    ba = float(np.max(squared(VB, VA, FA)[0]))
    return math.sqrt(max(ab, ba))


# ---- torch (fp64 on any device): the same operations, so the same bits ----------------------------------------------------
def _point_segment_torch(p, a, b):
    import torch
    ab = b - a
    t, l = rs._dt(p - a, ab), rs._dt(ab, ab)
    r = a + ab * (t / l)[..., None]
    r = torch.where((t >= l)[..., None], b, r)
    return torch.where((t <= 0)[..., None], a, r)


def point_face_torch(p, a, b, c):
    import torch
    r = rs.point_triangle_torch(p, a, b, c)
    ok = (area_term(a, b, c) > 0) & torch.isfinite(r).all(-1)
    if bool(ok.all()):
        return r
    s = _point_segment_torch(p, a, b)
    d = sq(p, s)
    for u, w in ((b, c), (c, a)):
        x = _point_segment_torch(p, u, w)
        e = sq(p, x)
        closer = e < d
        s = torch.where(closer[..., None], x, s)
        d = torch.where(closer, e, d)
    return torch.where(ok[..., None], r, s)


def squared_distance_torch(P, V, F, device="cpu", pchunk=1024, tchunk=4096):
    """squared_distance on a torch device, in chunks of points and faces: fp64 / int64 tensors on `device` (a later face chunk
    replaces the running best only when strictly closer: the lowest id wins a tie)"""
    import torch

    def f64(x):
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        return x.to(device=device, dtype=torch.float32).to(torch.float64)

    P, V = f64(P), f64(V)
    F = (F if isinstance(F, torch.Tensor) else torch.from_numpy(np.asarray(F, dtype=np.int64))).to(device=device, dtype=torch.int64)
    A, B, C = (V[F[:, k]] for k in range(3))
    T, n = F.shape[0], P.shape[0]
    sqrD = torch.empty(n, dtype=torch.float64, device=device)
    I = torch.empty(n, dtype=torch.int64, device=device)
    Cl = torch.empty((n, 3), dtype=torch.float64, device=device)
    for s in range(0, n, pchunk):
        p = P[s:s + pchunk, None, :]
        rows = torch.arange(p.shape[0], device=device)
        best_d = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=device)
        best_i = torch.zeros(p.shape[0], dtype=torch.int64, device=device)
        best_q = torch.zeros((p.shape[0], 3), dtype=torch.float64, device=device)
        for t in range(0, T, tchunk):
            q = point_face_torch(p, A[None, t:t + tchunk], B[None, t:t + tchunk], C[None, t:t + tchunk])
            d2 = sq(p, q)
            m = d2.min(dim=1).values
            ids = torch.arange(d2.shape[1], device=device)
            j = torch.where(d2 == m[:, None], ids, d2.shape[1]).min(dim=1).values
            better = m < best_d
            best_d = torch.where(better, m, best_d)
            best_i = torch.where(better, j + t, best_i)
            best_q = torch.where(better[:, None], q[rows, j], best_q)
        sqrD[s:s + pchunk], I[s:s + pchunk], Cl[s:s + pchunk] = best_d, best_i, best_q
    return sqrD, I, Cl


def squared_on(device, **chunks):
    """a `squared=` argument for hausdorff: squared_distance_torch on `device`, as numpy"""
    def squared(P, V, F):
        return tuple(x.cpu().numpy() for x in squared_distance_torch(P, V, F, device, **chunks))
    return squared
