"""
average_edge_length and massmatrix_voronoi (reference scripts/geometry.py:13-33, :35-89) restated in numpy, with their
gradients -- the checker of csrc/meshgeom.hip. fp64 by default; every function takes `dtype`.

Per face (corner k, k1 = k + 1 mod 3, k2 = k + 2 mod 3; l_k = length of the edge opposite corner k):
    cos_k   = (l_k1^2 + l_k2^2 - l_k^2) / (2 l_k1 l_k2)        law of cosines
    b_k     = cos_k l_k / (sum_j cos_j l_j)                    barycentric weights of the circumcentre
    A       = sqrt((l0 + l1 + l2)(l0 + l1 - l2)(l0 - l1 + l2)(-l0 + l1 + l2)) / 4     Heron
    cell_k  = (A b_k1 + A b_k2) / 2                            the quad of corner k up to the circumcentre
    obtuse corner k (cos_k < 0, tested for k = 0, 1, 2 in turn, a later one overrides): cell = A/2 at k, A/4 at the others
mass[v] = sum of the cells of v's corners: per corner slot j the corners in ascending face order, then (s0 + s1) + s2.
average_edge_length = (sum over faces of l0 + l1 + l2) / F / 3 -- interior edges count twice, boundary edges once.

The gradients replay the reverse pass of the reference's torch graph op by op (not a simplified closed form): where the
forward has special values (an exactly zero-length edge: NaN cells; an exactly collinear face: cos = +-1, sum_j cos_j l_j = 0,
A = 0) torch's backward rules decide the result -- d|x|/dx is 0 at x = 0, d sqrt(P) at P = 0 divides by zero, a torch.where
passes the gradient of the branch it selected and 0 (not 0 * NaN) to the other -- so the replay keeps them.
"""
import numpy as np


def _corners(v, f, dtype):
    v = np.asarray(v, dtype)
    f = np.asarray(f, np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def _norm(d, dtype):
    """|d| per row; in fp32 as torch's CPU norm(dim=1) evaluates it, sqrt(fma(z, z, fma(y, y, x * x))) -- each fp32 fma emulated
    in fp64, where the product is exact (one extra rounding, which can only matter on a tie)"""
    if dtype != np.float32:
        return np.sqrt((d * d).sum(1))
    x, y, z = (d[:, q].astype(np.float64) for q in range(3))
    t = (x * x).astype(np.float32).astype(np.float64)
    t = (y * y + t).astype(np.float32).astype(np.float64)
    return np.sqrt((z * z + t).astype(np.float32))


def reference_obtuse(v, f):
    """(F, 3) bool: cos_k < 0 as the reference evaluates it in fp32. A right angle rounds to a cosine of either sign (quad: the
    fp32 cosine is exactly 0, the fp64 one slightly negative), and the gradient differs between the two branches, so a check
    of fp32 results takes the branches from here."""
    return face_terms(v, f, np.float32)["obtuse"]


def vertex_condition(v, f):
    """(V,) the largest cancellation factor among a vertex's faces: Heron's (l0 + l1 + l2) / min of the three differences, and the
    barycentric sum's sum_k |cos_k l_k| / |sum_k cos_k l_k|. A rounding error of the fp32 arithmetic is amplified by up to
    this much (a noisy scan is full of needles: median 300 on the 1M-vertex noisy sphere)."""
    T = face_terms(v, f)
    s, l, cos = T["s"], T["l"], T["cos"]
    with np.errstate(all="ignore"):
        braw = np.abs(cos[0] * l[0]) + np.abs(cos[1] * l[1]) + np.abs(cos[2] * l[2])
        kap = np.maximum(s[0] / np.minimum(np.minimum(s[1], s[2]), s[3]), braw / np.abs(T["S"]))
    out = np.ones(np.asarray(v).shape[0])
    np.maximum.at(out, np.asarray(f, np.int64).reshape(-1), np.repeat(np.nan_to_num(kap, nan=np.inf), 3))
    return out


def face_terms(v, f, dtype=np.float64, obtuse=None):
    """every intermediate of one face's cells (dict of (F,) / (F, 3) arrays); obtuse: (F, 3) bool branch selection (None: cos_k < 0
    in `dtype`)"""
    p = _corners(v, f, dtype)
    with np.errstate(all="ignore"):
        d = [p[1] - p[2], p[2] - p[0], p[0] - p[1]]                   # edge opposite corner k
        l = [_norm(dk, dtype) for dk in d]
        sq = [lk * lk for lk in l]
        cos, den = [], []
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            den.append((2 * l[k1]) * l[k2])
            cos.append(((sq[k1] + sq[k2]) - sq[k]) / den[k])
        braw = [cos[k] * l[k] for k in range(3)]
        S = (braw[0] + braw[1]) + braw[2]
        bary = [braw[k] / S for k in range(3)]
        s = [(l[0] + l[1]) + l[2], (l[0] + l[1]) - l[2], (l[0] - l[1]) + l[2], (-l[0] + l[1]) + l[2]]
        P = ((s[0] * s[1]) * s[2]) * s[3]
        r = np.sqrt(P)
        A = 0.25 * r
        t = [A * bary[k] for k in range(3)]
        cells = np.stack([0.5 * (t[(k + 1) % 3] + t[(k + 2) % 3]) for k in range(3)], 1)
        obtuse = np.stack([c < 0 for c in cos], 1) if obtuse is None else np.asarray(obtuse, bool)
        for k in range(3):
            for j in range(3):
                cells[:, j] = np.where(obtuse[:, k], (0.5 if j == k else 0.25) * A, cells[:, j])
    return dict(p=p, d=d, l=l, cos=cos, den=den, S=S, bary=bary, s=s, r=r, A=A, cells=cells, obtuse=obtuse)


def massmatrix_voronoi(v, f, dtype=np.float64, obtuse=None):
    V = np.asarray(v).shape[0]
    f = np.asarray(f, np.int64)
    cells = face_terms(v, f, dtype, obtuse)["cells"]
    col = np.zeros((V, 3), dtype)
    for j in range(3):
        np.add.at(col[:, j], f[:, j], cells[:, j])      # unbuffered, in ascending face order
    with np.errstate(all="ignore"):
        return (col[:, 0] + col[:, 1]) + col[:, 2]


def massmatrix_voronoi_backward(v, f, g, dtype=np.float64, obtuse=None, magnitude=False):
    """d sum(g * massmatrix_voronoi(v, f)) / d v, (V, 3); magnitude: also the sum of |edge contributions| per vertex and coordinate
    (the scale of a rounding error in the per-vertex sum)"""
    V = np.asarray(v).shape[0]
    f = np.asarray(f, np.int64)
    T = face_terms(v, f, dtype, obtuse)
    g = np.asarray(g, dtype)
    G = [g[f[:, j]].copy() for j in range(3)]
    l, cos, den, bary, s, S, A = T["l"], T["cos"], T["den"], T["bary"], T["s"], T["S"], T["A"]
    with np.errstate(all="ignore"):
        gA = np.zeros_like(A)
        for k in (2, 1, 0):                                  # the overrides, last applied first
            m = T["obtuse"][:, k]
            for j in (2, 1, 0):
                gA = gA + (0.5 if j == k else 0.25) * np.where(m, G[j], 0)
                G[j] = np.where(m, 0, G[j])
        gt = [0.5 * G[(k + 1) % 3] + 0.5 * G[(k + 2) % 3] for k in range(3)]   # t_k enters the cells of k1 and k2
        gl = [np.zeros_like(A) for _ in range(3)]
        gbraw, gS = [], np.zeros_like(A)
        for k in range(3):
            gA = gA + gt[k] * bary[k]
            gb = gt[k] * A
            gbraw.append(gb / S)
            gS = gS - gb * (bary[k] / S)
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            gbr = gbraw[k] + gS
            gcos = gbr * l[k]
            gl[k] = gl[k] + gbr * cos[k]
            gnum = gcos / den[k]
            gden = -gcos * (cos[k] / den[k])
            gl[k1] = gl[k1] + 2 * (gden * l[k2]) + 2 * gnum * l[k1]
            gl[k2] = gl[k2] + gden * (2 * l[k1]) + 2 * gnum * l[k2]
            gl[k] = gl[k] - 2 * gnum * l[k]
        gP = (0.25 * gA) / (2 * T["r"])
        gs3 = gP * ((s[0] * s[1]) * s[2])
        g012 = gP * s[3]
        gs2 = g012 * (s[0] * s[1])
        g01 = g012 * s[2]
        gs0, gs1 = g01 * s[1], g01 * s[0]
        gl[0] = gl[0] + gs0 + gs1 + gs2 - gs3
        gl[1] = gl[1] + gs0 + gs1 - gs2 + gs3
        gl[2] = gl[2] + gs0 - gs1 + gs2 + gs3
        return _edges_to_verts(V, f, T["d"], [np.where(l[k] == 0, 0, gl[k] / l[k]) for k in range(3)], dtype, magnitude)


def _edges_to_verts(V, f, d, c, dtype, magnitude=False):
    """d_k = p[k1] - p[k2] with gradient c_k d_k: + to corner k1, - to corner k2"""
    out, mag = np.zeros((V, 3), dtype), np.zeros((V, 3), dtype)
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        gd = d[k] * c[k][:, None]
        np.add.at(out, f[:, k1], gd)
        np.add.at(out, f[:, k2], -gd)
        if magnitude:
            np.add.at(mag, f[:, k1], np.abs(gd))
            np.add.at(mag, f[:, k2], np.abs(gd))
    return (out, mag) if magnitude else out


def average_edge_length(v, f, dtype=np.float64):
    T = face_terms(v, f, dtype)
    with np.errstate(all="ignore"):
        return ((T["l"][0] + T["l"][1]) + T["l"][2]).sum() / np.asarray(f).shape[0] / 3


def average_edge_length_backward(v, f, g=1.0, dtype=np.float64, magnitude=False):
    """d (g * average_edge_length(v, f)) / d v, (V, 3); magnitude: as in massmatrix_voronoi_backward"""
    V = np.asarray(v).shape[0]
    f = np.asarray(f, np.int64)
    T = face_terms(v, f, dtype)
    c = dtype(g) / 3 / f.shape[0]
    with np.errstate(all="ignore"):
        return _edges_to_verts(V, f, T["d"], [np.where(lk == 0, 0, c / lk) for lk in T["l"]], dtype, magnitude)
