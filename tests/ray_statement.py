"""
Statement of the ray query of largesteps.raycast (csrc/raycast.hip): a numpy fp64 brute force over all faces with
the operations of the device code in its order (the build has -ffp-contract=off, so the device returns the same bits).

1. Ray. Origin o and direction d are fp32, widened to fp64; d need not be unit. A d with a non-finite component, or all zero, hits
   nothing. Otherwise kz is the axis of largest |d| (the lowest on a tie), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky swapped when
   d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
2. Face (a, b, c). A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz]; B and C likewise. U = Cx By - Cy Bx, V = Ax Cy - Ay Cx,
   W = Bx Ay - By Ax, det = (U + V) + W. The face is hit iff U, V, W are all >= 0 or all <= 0, and det != 0: edges and vertices count, and a
   NaN fails every comparison. t = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det; the hit is accepted iff tmin <= t <= tmax; the
   weights of (a, b, c) are (U / det, V / det, W / det).
3. Result. Closest hit: the accepted face of smallest t, the lowest id on equal t; a miss is t = +inf, I = -1, W = 0. Any hit: some face
   is accepted.
4. Gradient of t, the face held fixed. ab = b - a, ac = c - a, n = (ab_y ac_z - ab_z ac_y, ab_z ac_x - ab_x ac_z, ab_x ac_y - ab_y ac_x),
   nd = (n_x d_x + n_y d_y) + n_z d_z, q = n / nd. With g the incoming gradient: the term to o is -(g q), to d -((g t) q), to corner k
   (g w_k) q, each rounded to fp32 once; a ray whose I is outside [0, F) has zero terms. The vertex gradient adds the corner terms in the
   order of distance_grad_statement (keys / face_rows / vertex_sums).
"""
import numpy as np


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def frame(D):
    """rule 1: (ok (n,), kx, ky, kz (n,), Sx, Sy, Sz (n,)) of the fp64 directions D (n, 3)"""
    ok = np.isfinite(D).all(1) & (np.abs(D) > 0).any(1)
    a = np.abs(np.where(np.isfinite(D), D, 0.0))
    kz = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    r = np.arange(D.shape[0])
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = D[r, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(divide="ignore", invalid="ignore"):
        dz = D[r, kz]
        return ok, kx, ky, kz, D[r, kx] / dz, D[r, ky] / dz, 1.0 / dz


def faces_of_rays(O, D, V, F):
    """rule 2 for every (ray, face) pair: (hit (n, m) bool before the range test, t (n, m), U, V, W, det (n, m)). The rays are handled
    in groups of one (kx, ky, kz), so that an axis is a column"""
    O, D, V, F = _f64(O), _f64(D), _f64(V), np.asarray(F, dtype=np.int64)
    ok, kx, ky, kz, Sx, Sy, Sz = frame(D)
    n, m = O.shape[0], F.shape[0]
    out = [np.zeros((n, m), dtype=bool)] + [np.full((n, m), np.nan) for _ in range(5)]
    corners = [V[F[:, c]] for c in range(3)]
    for x, y, z in sorted(set(zip(kx.tolist(), ky.tolist(), kz.tolist()))):
        g = np.nonzero((kx == x) & (ky == y) & (kz == z))[0]
        sx, sy, sz = Sx[g, None], Sy[g, None], Sz[g, None]

        def shear(P):
            px, py, pz = P[None, :, x] - O[g, None, x], P[None, :, y] - O[g, None, y], P[None, :, z] - O[g, None, z]
            return px - sx * pz, py - sy * pz, pz
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            Ax, Ay, Az = shear(corners[0])
            Bx, By, Bz = shear(corners[1])
            Cx, Cy, Cz = shear(corners[2])
            U = Cx * By - Cy * Bx
            Vv = Ax * Cy - Ay * Cx
            W = Bx * Ay - By * Ax
            det = (U + Vv) + W
            hit = (((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))) & (det != 0) & ok[g, None]
            t = ((U * (sz * Az) + Vv * (sz * Bz)) + W * (sz * Cz)) / det
        for dst, src in zip(out, (hit, t, U, Vv, W, det)):
            dst[g] = src
    return tuple(out)


def _range(trange, n):
    if trange is None:
        return np.zeros(n), np.full(n, np.inf)
    trange = np.asarray(trange, dtype=np.float64)
    return trange[:, 0], trange[:, 1]


def closest(O, D, V, F, trange=None, chunk=256):
    """rule 3: (t (n,) fp64, I (n,) int64, W (n, 3) fp64), chunked over the rays"""
    n = np.asarray(O).shape[0]
    tmin, tmax = _range(trange, n)
    t_out, I_out, W_out = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.zeros((n, 3))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        hit, t, U, Vv, W, det = faces_of_rays(np.asarray(O)[s:e], np.asarray(D)[s:e], V, F)
        with np.errstate(invalid="ignore"):
            acc = hit & (t >= tmin[s:e, None]) & (t <= tmax[s:e, None])
        key = np.where(acc, t, np.inf)
        best = key.min(1)
        first = (acc & (key == best[:, None])).argmax(1)                 # the lowest id among the accepted faces of smallest t
        any_ = acc.any(1)
        r = np.arange(e - s)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.stack([U[r, first], Vv[r, first], W[r, first]], -1) / det[r, first][:, None]
        t_out[s:e] = np.where(any_, t[r, first], np.inf)
        I_out[s:e] = np.where(any_, first, -1)
        W_out[s:e] = np.where(any_[:, None], w, 0.0)
    return t_out, I_out, W_out


def any_hit(O, D, V, F, trange=None, chunk=256):
    """rule 3: (n,) bool"""
    n = np.asarray(O).shape[0]
    tmin, tmax = _range(trange, n)
    out = np.zeros(n, dtype=bool)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        hit, t, *_ = faces_of_rays(np.asarray(O)[s:e], np.asarray(D)[s:e], V, F)
        with np.errstate(invalid="ignore"):
            out[s:e] = (hit & (t >= tmin[s:e, None]) & (t <= tmax[s:e, None])).any(1)
    return out


def terms(O, D, V, F, I, W, t, g):
    """rule 4 before the rounding: (tO (n, 3), tD (n, 3), tV (n, 3 corners, 3)) fp64; zeros for an I outside [0, F)"""
    D, V, F = _f64(D), _f64(V), np.asarray(F, dtype=np.int64)
    I, W, t, g = np.asarray(I, dtype=np.int64), np.asarray(W, dtype=np.float64), np.asarray(t, dtype=np.float64), np.asarray(g, dtype=np.float64)
    ok = (I >= 0) & (I < F.shape[0])
    f = F[np.where(ok, I, 0)]
    a, b, c = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    ab, ac = b - a, c - a
    nrm = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nd = (nrm[:, 0] * D[:, 0] + nrm[:, 1] * D[:, 1]) + nrm[:, 2] * D[:, 2]
        q = nrm / nd[:, None]
        tO = -(g[:, None] * q)
        tD = -((g * t)[:, None] * q)
        tV = (g[:, None] * W)[:, :, None] * q[:, None, :]
    z = ~ok
    tO[z], tD[z], tV[z] = 0.0, 0.0, 0.0
    return tO, tD, tV


def closest_torch(O, D, V, F, trange, dev, chunk=64):
    """rules 1-3 with the same operations as torch fp64 tensors on `dev`, for meshes too large for numpy: (t, I, W) tensors. Every
    operation is one IEEE fp64 elementwise kernel, so the bits are those of `closest` (the device test checks that on small meshes)"""
    import torch
    O64, D64 = _f64(O), _f64(D)
    ok, kx, ky, kz, Sx, Sy, Sz = frame(D64)
    n = O64.shape[0]
    tmin, tmax = _range(trange, n)
    tV = torch.from_numpy(_f64(V)).to(dev)
    tF = torch.from_numpy(np.asarray(F, dtype=np.int64)).to(dev)
    corners = [tV[tF[:, c]] for c in range(3)]
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                 # noqa: E731
    t_out = torch.full((n,), np.inf, dtype=torch.float64, device=dev)
    I_out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    W_out = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    for x, y, z in sorted(set(zip(kx.tolist(), ky.tolist(), kz.tolist()))):
        group = np.nonzero((kx == x) & (ky == y) & (kz == z))[0]
        for s in range(0, group.size, chunk):
            g = group[s:s + chunk]
            o, sx, sy, sz = dv(O64[g]), dv(Sx[g, None]), dv(Sy[g, None]), dv(Sz[g, None])

            def shear(P):
                px, py, pz = P[None, :, x] - o[:, None, x], P[None, :, y] - o[:, None, y], P[None, :, z] - o[:, None, z]
                return px - sx * pz, py - sy * pz, pz
            Ax, Ay, Az = shear(corners[0])
            Bx, By, Bz = shear(corners[1])
            Cx, Cy, Cz = shear(corners[2])
            U = Cx * By - Cy * Bx
            Vv = Ax * Cy - Ay * Cx
            W = Bx * Ay - By * Ax
            det = (U + Vv) + W
            hit = (((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))) & (det != 0) & dv(ok[g, None])
            t = ((U * (sz * Az) + Vv * (sz * Bz)) + W * (sz * Cz)) / det
            acc = hit & (t >= dv(tmin[g, None])) & (t <= dv(tmax[g, None]))
            key = torch.where(acc, t, torch.full_like(t, np.inf))
            best = key.min(1).values
            # the lowest id among the accepted faces of smallest t (torch's argmax promises no order among equal values)
            idx = torch.arange(t.shape[1], device=dev)[None, :].expand_as(t)
            first = torch.where(acc & (key == best[:, None]), idx, torch.full_like(idx, t.shape[1])).min(1).values.clamp_max(t.shape[1] - 1)
            any_ = acc.any(1)
            r = torch.arange(g.size, device=dev)
            w = torch.stack([U[r, first], Vv[r, first], W[r, first]], -1) / det[r, first][:, None]
            tg = dv(g)
            t_out[tg] = torch.where(any_, t[r, first], torch.full_like(best, np.inf))
            I_out[tg] = torch.where(any_, first, torch.full_like(first, -1))
            W_out[tg] = torch.where(any_[:, None], w, torch.zeros_like(w))
    return t_out, I_out, W_out
