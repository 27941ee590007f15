"""
Statement of the self-intersection query of largesteps.distance (csrc/selfx.hip): numpy fp64 with the operations
of the device code in its order (the build has -ffp-contract=off), as a brute force over all pairs of faces. No device.

1. Segment against face. p, q and the corners a, b, c are fp32, widened to fp64. The segment (p, q) crosses the face (a, b, c) iff the ray
   rule of tests/ray_statement.py, with the origin o = p and the direction d = q - p formed in fp64 (not rounded to fp32), accepts the face
   with 0 <= t <= 1: kz is the axis of largest |d| (the lowest on a tie), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky swapped when
   d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; A = a - p, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], B and C
   likewise; U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax, det = (U + V) + W; the face is hit iff U, V, W are all >= 0 or all
   <= 0, and det != 0; t = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det. Edges and vertices count; det == 0 never hits (a zero-area
   face, a segment in the face's plane); a d that is all zero or has a non-finite component hits nothing.
2. Face pairs. For faces f < g, s is the number of equal (corner of f, corner of g) index pairs among the nine: for faces without a
   repeated index, the number of vertex indices they share. Edge e of a face goes from corner e to corner (e + 1) % 3.
     s >= 2: never reported (edge neighbours, duplicates).
     s == 1, corner i of f being corner j of g: reported iff edge (i + 1) % 3 of f (the one opposite corner i) crosses g, or edge
             (j + 1) % 3 of g crosses f.
     s == 0: reported iff one of the three edges of f crosses g, or one of the three edges of g crosses f.
3. The box clause. A pair is reported only if the corner boxes of f and g are within 2 e of each other on all three axes. The corner
   box of a face is the smallest and largest of its three fp32 corners per axis (fmin / fmax: a NaN corner is passed over), widened to
   fp64; e = 2^-40 x the largest |coordinate| of V (every row, referenced by a face or not; a NaN coordinate is passed over here as
   in the boxes; the product is exact). On an axis the boxes
   are apart iff lo_g - e > hi_f + e or hi_g + e < lo_f - e, each side rounded once in fp64; a comparison with a NaN is false, so such a
   pair is not apart. The clause is symmetric in f and g. Where rule 2 accepts with numbers that mean something, the segment passes
   within a few fp64 roundings of the face, far inside e, and the clause changes nothing; it decides the pairs rule 2 accepts on rounding
   alone: on an exactly flat sheet whose shear rounds, U = W = 0 and det = V = a rounding error, and t comes out in [0, 1] for faces any
   distance apart in the sheet's plane.
4. Result. IF (k, 2) int64: the reported pairs (f, g), f < g, sorted lexicographically.

What follows: coplanar overlaps are not reported (a sheet folded flat onto itself) where det == 0 is exact; in a tilted plane whose shear
rounds, rule 1 decides coplanar faces on a rounding error and rule 3 keeps the near ones of them (tilted_flat_overlap below): arbitrary,
but a function of the mesh, and the same on the device; two faces without a common index that touch at a point or along a segment are; an edge through the common edge of two faces is reported against at least one of them (an edge function
depends on the segment and the two sheared ends only, and swapping the ends negates it exactly).
"""
import numpy as np


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def cross_rows(P, Q, A, B, C):
    """rule 1 for n rows at once: (n,) bool, all arguments (n, 3) fp64"""
    n = P.shape[0]
    D = Q - P
    ok = np.isfinite(D).all(1) & (np.abs(D) > 0).any(1)
    a = np.abs(np.where(np.isfinite(D), D, 0.0))
    kz = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    r = np.arange(n)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = D[r, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dz = D[r, kz]
        Sx, Sy, Sz = D[r, kx] / dz, D[r, ky] / dz, 1.0 / dz

        def shear(X):
            x, y, z = X[r, kx] - P[r, kx], X[r, ky] - P[r, ky], X[r, kz] - P[r, kz]
            return x - Sx * z, y - Sy * z, z
        Ax, Ay, Az = shear(A)
        Bx, By, Bz = shear(B)
        Cx, Cy, Cz = shear(C)
        U = Cx * By - Cy * Bx
        Vv = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        det = (U + Vv) + W
        hit = (((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))) & (det != 0) & ok
        t = ((U * (Sz * Az) + Vv * (Sz * Bz)) + W * (Sz * Cz)) / det
        return hit & (t >= 0) & (t <= 1)


def crosses(p, q, a, b, c):
    """rule 1: does the segment (p, q) cross the face (a, b, c)"""
    return bool(cross_rows(*(_f64(x).reshape(1, 3) for x in (p, q, a, b, c)))[0])


def slack(V):
    """e of rule 3: 2^-40 x the largest |coordinate| of V, a NaN passed over (0 when every coordinate is one)"""
    return 2.0 ** -40 * float(np.fmax.reduce(np.abs(_f64(V)).reshape(-1), initial=0.0))


def boxes_near(V, F, fi, gi):
    """rule 3 for the candidate pairs (fi[r], gi[r]): (n,) bool, False where the corner boxes are apart on some axis"""
    V64, F = _f64(V), np.asarray(F, dtype=np.int64)
    e = slack(V)
    with np.errstate(invalid="ignore"):
        C = V64[F]
        lo = np.fmin(np.fmin(C[:, 0], C[:, 1]), C[:, 2])
        hi = np.fmax(np.fmax(C[:, 0], C[:, 1]), C[:, 2])
        apart = (lo[gi] - e > hi[fi] + e) | (hi[gi] + e < lo[fi] - e)
    return ~apart.any(1)


def rule(V, F, fi, gi, box_clause=True):
    """rules 2 and 3 for the candidate pairs (fi[r], gi[r]), fi < gi: (n,) bool, reported or not. box_clause=False is rule 2 alone, for
    the tests that show what rule 3 decides"""
    near = boxes_near(V, F, fi, gi) if box_clause else np.ones(len(fi), dtype=bool)
    V, F = _f64(V), np.asarray(F, dtype=np.int64)
    Ff, Fg = F[fi], F[gi]
    n = Ff.shape[0]
    M = Ff[:, :, None] == Fg[:, None, :]
    s = M.sum((1, 2))
    need = np.zeros((n, 6), dtype=bool)                      # tests 0..2: the edges of f against g, 3..5: those of g against f
    need[s == 0] = True
    one = np.nonzero(s == 1)[0]
    need[one, (M[one].any(2).argmax(1) + 1) % 3] = True
    need[one, 3 + (M[one].any(1).argmax(1) + 1) % 3] = True
    need &= near[:, None]
    rep = np.zeros(n, dtype=bool)
    for test in range(6):
        src, dst = (Ff, Fg) if test < 3 else (Fg, Ff)
        e = test % 3
        rows = np.nonzero(need[:, test] & ~rep)[0]
        if rows.size:
            rep[rows] = cross_rows(V[src[rows, e]], V[src[rows, (e + 1) % 3]], V[dst[rows, 0]], V[dst[rows, 1]], V[dst[rows, 2]])
    return rep


def _sorted(out):
    IF = np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
    return IF[np.lexsort((IF[:, 1], IF[:, 0]))]


def pairs(V, F, chunk=256):
    """rules 2 to 4 over all f < g, `chunk` faces f at a time"""
    m = np.asarray(F).shape[0]
    out = []
    for s in range(0, m, chunk):
        fi, gi = np.meshgrid(np.arange(s, min(m, s + chunk)), np.arange(m), indexing="ij")
        keep = fi < gi
        fi, gi = fi[keep], gi[keep]
        rep = rule(V, F, fi, gi)
        out.append(np.stack([fi[rep], gi[rep]], 1).astype(np.int64))
    return _sorted(out)


def pairs_fast(V, F, chunk=256):
    """the same rules applied only to the pairs whose exact corner boxes, each widened by 1e-6 x the largest side of the mesh's box
    (and by 2 e, so that no pair of rule 3 is lost on a mesh far from the origin), overlap: for the larger cases. The candidates are a
    superset of the pairs that pass rule 3, which `rule` applies itself, so the result is that of `pairs` on every mesh."""
    V64, F = _f64(V), np.asarray(F, dtype=np.int64)
    m = F.shape[0]
    w = 1e-6 * float((V64.max(0) - V64.min(0)).max()) + 2.0 * slack(V)
    with np.errstate(invalid="ignore"):
        C = V64[F]
        lo = np.fmin(np.fmin(C[:, 0], C[:, 1]), C[:, 2]) - w
        hi = np.fmax(np.fmax(C[:, 0], C[:, 1]), C[:, 2]) + w
    out = []
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        near = ~((lo[s:e, None, :] > hi[None, :, :]) | (lo[None, :, :] > hi[s:e, None, :])).any(2)
        fi, gi = np.nonzero(near)
        fi = fi + s
        keep = fi < gi
        fi, gi = fi[keep], gi[keep]
        rep = rule(V, F, fi, gi)
        out.append(np.stack([fi[rep], gi[rep]], 1).astype(np.int64))
    return _sorted(out)


def shares_a_vertex(F, IF):
    """(k,) bool: the pairs of IF whose faces have an index in common"""
    F = np.asarray(F, dtype=np.int64)
    return (F[IF[:, 0]][:, :, None] == F[IF[:, 1]][:, None, :]).any((1, 2))


# ---- the meshes of the tests (fp32 V, int64 F) -----------------------------------------------------------------------------------------
F32 = np.float32
_A = [[0, 0, 0], [2, 0, 0], [0, 2, 0]]                       # the face every hand case starts from, in the plane z = 0

HAND_CASES = {   # name -> (V, F, expected number of pairs)
    "crossing": (_A + [[0.5, 0.5, -1], [0.5, 0.5, 1], [1.5, 1.5, 0.5]], [[0, 1, 2], [3, 4, 5]], 1),
    "ends_on_the_plane": (_A + [[0.5, 0.5, 0], [0.5, 0.5, 1], [1.5, 0.5, 1]], [[0, 1, 2], [3, 4, 5]], 1),
    "coplanar_overlap": (_A + [[0.5, 0.5, 0], [2.5, 0.5, 0], [0.5, 2.5, 0]], [[0, 1, 2], [3, 4, 5]], 0),
    "shared_vertex_piercing": (_A + [[0.5, 0.5, -1], [0.5, 0.5, 1]], [[0, 1, 2], [0, 3, 4]], 1),
    "shared_vertex_clean": (_A + [[-1, 0, 1], [0, -1, 1]], [[0, 1, 2], [0, 3, 4]], 0),
    "shared_edge_and_duplicates": (_A + [[1, 1, 1]], [[0, 1, 2], [1, 0, 3], [0, 1, 2], [2, 0, 1]], 0),
}


def hand_case(name):
    v, f, k = HAND_CASES[name]
    return np.array(v, dtype=F32), np.array(f, dtype=np.int64), k


def jittered(n, tangential, seed=5):
    """icosphere(n) with perturb(V, tangential=tangential, edge=mean |V[F0] - V[F1]|, seed=seed)"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(n)
    edge = float(np.linalg.norm(v[f[:, 0]].astype(np.float64) - v[f[:, 1]].astype(np.float64), axis=1).mean())
    return synthetic.perturb(v, tangential=tangential, edge=edge, seed=seed).astype(F32), np.asarray(f, dtype=np.int64)


def two_spheres(n=4, offset=(0.37, 0.11, 0.05)):
    """icosphere(n) and a copy of it moved by `offset`, as one mesh of two components"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(n)
    f = np.asarray(f, dtype=np.int64)
    return np.concatenate([v, (v.astype(np.float64) + np.array(offset)).astype(F32)]).astype(F32), np.concatenate([f, f + v.shape[0]])


def tilted_flat_sheet(n=12, step=1.0 / 16.0):
    """plane(n)'s faces over the lattice x = i step, y = j step in the plane z = x + 3 y. With step = 1/16 every coordinate is exact in
    fp32 and the sheet is exactly flat; the shear of rule 1 rounds, so rule 2 alone accepts faces lattice steps apart (module docstring,
    rule 3). step = 1/11 is the same sheet with rounded coordinates."""
    from largesteps import synthetic
    v, f = synthetic.plane(n, dtype=np.float64)
    i, j = np.rint(v[:, 0] * (n - 1)), np.rint(v[:, 1] * (n - 1))
    x, y = i * step, j * step
    return np.stack([x, y, x + 3.0 * y], 1).astype(F32), np.asarray(f, dtype=np.int64)


def pierced_flat_sheet():
    """tilted_flat_sheet() and, as the last face, a triangle with an edge through it: real pairs among the ones rule 3 removes"""
    v, f = tilted_flat_sheet()
    k = v.shape[0]
    tri = F32([[0.3, 0.3, 0.5], [0.33, 0.31, 2.0], [0.9, 0.9, 1.0]])
    return np.concatenate([v, tri]), np.concatenate([f, [[k, k + 1, k + 2]]])


def tilted_flat_overlap():
    """tilted_flat_sheet() and a copy of it moved by half a cell inside its own plane, exactly: coplanar faces that overlap, in a plane
    where the shear rounds. Rule 2 decides such pairs on rounding, rule 3 keeps the near ones of them: what the rules say of coplanar
    faces in a tilted plane is arbitrary, but it is a function of the mesh, and the device must say the same."""
    v, f = tilted_flat_sheet()
    x, y = v[:, 0].astype(np.float64) + 1.0 / 32.0, v[:, 1].astype(np.float64) + 1.0 / 32.0
    return np.concatenate([v, np.stack([x, y, x + 3.0 * y], 1).astype(F32)]), np.concatenate([f, f + v.shape[0]])


def cutting_fold(n=12):
    """plane(n) folded along x = 1/2 with the second layer tilted about the line y = 0.275, so that it cuts through the first"""
    from largesteps import synthetic
    v, f = synthetic.plane(n, dtype=np.float64)
    x, y = v[:, 0], v[:, 1]
    second = x > 0.5
    xx = np.where(second, 1.0 - x, x)
    z = 0.1 * np.sin(2.0 * np.pi * xx) + np.where(second, 0.07 * (2.0 * y - 0.55), 0.0)
    return np.stack([xx, y, z], 1).astype(F32), np.asarray(f, dtype=np.int64)
