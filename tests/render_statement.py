"""
Numpy statement of the differentiable rasterizer of csrc/raster.hip (largesteps.render): rasterize, interpolate and antialias, forward
and backward. It is the specification.

- Coverage is decided with the kernel's fp64 homogeneous edge functions in the kernel's operation order, so the triangle-id map is
  bit-identical; u, v and z/w come from the same fp64 quantities rounded once to fp32 (the kernel agrees to within 1 ulp, in
  practice 0). `clip_cover` restates the near / far handling by an independent method -- Sutherland-Hodgman clipping of the triangle
  in homogeneous space against z = -w and z = w, then a point-in-polygon test -- for the tests to compare against away from edges.
- interpolate and antialias follow the kernel's fp32 operation order; the backwards are the analytic derivatives of the forwards
  (fp64 here; the kernel sums in another fixed order, so they agree to rounding, not bitwise).
- nvdiffrast is not available on this hardware, so parity with it cannot be pinned: the conventions (rast = (u, v, z/w, id + 1),
  background 0, row 0 at NDC y = -1, pixel centres at ((2x + 1) / W - 1, (2y + 1) / H - 1), interpolation u a0 + v a1 + (1 - u - v) a2)
  are nvdiffrast's documented ones as far as they can be stated without it. The antialias blend rule is this project's own.
"""
import numpy as np

F32 = np.float32


def _cross(a, b):
    """fp64 cross product over (x, y, w) of fp32 rows a, b (..., 4) -- the kernel's rs_cross"""
    ax, ay, aw = a[..., 0].astype(np.float64), a[..., 1].astype(np.float64), a[..., 3].astype(np.float64)
    bx, by, bw = b[..., 0].astype(np.float64), b[..., 1].astype(np.float64), b[..., 3].astype(np.float64)
    return np.stack([ay * bw - aw * by, aw * bx - ax * bw, ax * by - ay * bx], axis=-1)


def setup(q):
    """q (3, 4) fp32 clip-space corners -> (c (3, 3), D)"""
    c = np.stack([_cross(q[1], q[2]), _cross(q[2], q[0]), _cross(q[0], q[1])])
    D = (np.float64(q[0, 0]) * c[0, 0] + np.float64(q[0, 1]) * c[0, 1]) + np.float64(q[0, 3]) * c[0, 2]
    return c, D


def centres(n):
    return (2.0 * np.arange(n, dtype=np.float64) + 1.0) / np.float64(n) - 1.0


def cover(q, px, py):
    """coverage of the pixel centres (px, py) (fp64 arrays) by the triangle q: (mask, E (3, ...), zf fp32)"""
    c, D = setup(q)
    s = 1.0 if D > 0.0 else -1.0
    E = np.stack([(px * c[i, 0] + py * c[i, 1]) + c[i, 2] for i in range(3)])
    inside = np.ones(np.shape(px), dtype=bool)
    for i in range(3):
        e = s * E[i]
        cx, cy = s * c[i, 0], s * c[i, 1]
        inside &= (e > 0.0) | ((e == 0.0) & ((cx > 0.0) | ((cx == 0.0) & (cy > 0.0))))
    S = (E[0] + E[1]) + E[2]
    with np.errstate(all="ignore"):
        inside &= s * S > 0.0
        zw = ((np.float64(q[0, 2]) * E[0] + np.float64(q[1, 2]) * E[1]) + np.float64(q[2, 2]) * E[2]) / D
        zf = zw.astype(F32)
    inside &= (zf >= F32(-1.0)) & (zf <= F32(1.0))
    if not (D != 0.0) or np.isnan(D):
        inside[...] = False
    return inside, E, zf


def _order_bits(z):
    u = np.asarray(z, dtype=F32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def rasterize(pos, tri, H, W):
    """pos (B, V, 4) fp32, tri (F, 3) -> rast (B, H, W, 4) fp32"""
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    B = pos.shape[0]
    py, px = np.meshgrid(centres(H), centres(W), indexing="ij")
    rast = np.zeros((B, H, W, 4), dtype=F32)
    for b in range(B):
        best = np.full((H, W), np.iinfo(np.uint64).max, dtype=np.uint64)
        for f in range(tri.shape[0]):
            q = pos[b, tri[f]]
            m, E, zf = cover(q, px, py)
            if not m.any():
                continue
            key = (_order_bits(zf) << np.uint64(32)) | np.uint64(f)
            best = np.where(m, np.minimum(best, key), best)
        hit = best != np.iinfo(np.uint64).max
        ids = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
        for f in np.unique(ids[hit]):
            m = hit & (ids == f)
            _, E, zf = cover(pos[b, tri[f]], px[m], py[m])
            S = (E[0] + E[1]) + E[2]
            rast[b][m] = np.stack([(E[0] / S).astype(F32), (E[1] / S).astype(F32), zf, np.full(m.sum(), f + 1, F32)], axis=-1)
    return rast


def clip_cover(q, px, py):
    """Independent near / far handling: clip the triangle against -w <= z <= w (and w > 0) in homogeneous space, project, and test the
    pixel centres against the resulting convex polygon (no tie rule: use away from edges)"""
    poly = [np.asarray(v, dtype=np.float64) for v in q]
    for sgn in (1.0, -1.0):                       # z + w >= 0 (near), w - z >= 0 (far)
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = a[3] + sgn * a[2], b[3] + sgn * b[2]
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                t = da / (da - db)
                out.append(a + t * (b - a))
        poly = out
        if not poly:
            return np.zeros(np.shape(px), dtype=bool)
    if any(v[3] <= 0 for v in poly):
        return np.zeros(np.shape(px), dtype=bool)
    P = np.array([[v[0] / v[3], v[1] / v[3]] for v in poly])
    n = len(P)
    area = sum(P[i, 0] * P[(i + 1) % n, 1] - P[(i + 1) % n, 0] * P[i, 1] for i in range(n))
    m = np.ones(np.shape(px), dtype=bool)
    for i in range(n):
        a, b = P[i], P[(i + 1) % n]
        e = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        m &= e * np.sign(area) > 0
    return m


def rasterize_backward(pos, tri, rast, g_rast):
    """d sum(g_rast[..., 0] u + g_rast[..., 1] v) / d pos, (B, V, 4) fp64, [..., 2] = 0"""
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    gp = np.zeros(pos.shape, dtype=np.float64)
    cw, ch = centres(W), centres(H)
    for b in range(B):
        ys, xs = np.nonzero(rast[b, :, :, 3])
        for y, x in zip(ys, xs):
            f = int(rast[b, y, x, 3]) - 1
            q = pos[b, tri[f]]
            c, D = setup(q)
            p = np.array([cw[x], ch[y], 1.0])
            E = c @ p
            S = E.sum()
            gu, gv = float(g_rast[b, y, x, 0]), float(g_rast[b, y, x, 1])
            dot = gu * E[0] / S + gv * E[1] / S
            dE = np.array([gu - dot, gv - dot, -dot]) / S
            Q = q[:, [0, 1, 3]].astype(np.float64)
            for j in range(3):
                g = dE[(j + 2) % 3] * np.cross(Q[(j + 1) % 3], p) + dE[(j + 1) % 3] * np.cross(p, Q[(j + 2) % 3])
                gp[b, tri[f, j], [0, 1, 3]] += g
    return gp


def interpolate(attr, rast, tri):
    attr = np.asarray(attr, dtype=F32)
    if attr.ndim == 2:
        attr = attr[None]
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    C = attr.shape[2]
    out = np.zeros((B, H, W, C), dtype=F32)
    for b in range(B):
        a = attr[0 if attr.shape[0] == 1 else b]
        ids = rast[b, :, :, 3].astype(np.int64)
        m = ids > 0
        t = tri[ids[m] - 1]
        u, v = rast[b, :, :, 0][m][:, None], rast[b, :, :, 1][m][:, None]
        w = (F32(1.0) - u) - v
        out[b][m] = (u * a[t[:, 0]] + v * a[t[:, 1]]) + w * a[t[:, 2]]
    return out


def interpolate_backward(attr, rast, tri, g):
    """(grad_attr shaped like attr, grad_rast (B, H, W, 4)) in fp64"""
    attr = np.asarray(attr, dtype=F32)
    shape = attr.shape
    a3 = attr[None] if attr.ndim == 2 else attr
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    ga = np.zeros(a3.shape, dtype=np.float64)
    gr = np.zeros((B, H, W, 4), dtype=np.float64)
    for b in range(B):
        bb = 0 if a3.shape[0] == 1 else b
        ids = rast[b, :, :, 3].astype(np.int64)
        ys, xs = np.nonzero(ids)
        for y, x in zip(ys, xs):
            t = tri[ids[y, x] - 1]
            u, v = np.float64(rast[b, y, x, 0]), np.float64(rast[b, y, x, 1])
            gg = g[b, y, x].astype(np.float64)
            ga[bb, t[0]] += u * gg
            ga[bb, t[1]] += v * gg
            ga[bb, t[2]] += (1.0 - u - v) * gg
            gr[b, y, x, 0] = (gg * (a3[bb, t[0]] - a3[bb, t[2]])).sum()
            gr[b, y, x, 1] = (gg * (a3[bb, t[1]] - a3[bb, t[2]])).sum()
    return ga.reshape(shape), gr


# ---- antialias --------------------------------------------------------------------------------------------------------------------
def adjacency(tri):
    """adj (F, 3): the face across edge (corner e, corner e + 1), -1 for an edge with one face or more than two"""
    tri = np.asarray(tri, dtype=np.int64)
    F = tri.shape[0]
    edges = {}
    for f in range(F):
        for e in range(3):
            a, b = tri[f, e], tri[f, (e + 1) % 3]
            edges.setdefault((min(a, b), max(a, b)), []).append((f, e))
    adj = -np.ones((F, 3), dtype=np.int64)
    for hs in edges.values():
        if len(hs) == 2:
            (f0, e0), (f1, e1) = hs
            adj[f0, e0], adj[f1, e1] = f1, f0
    return adj


def _det(q):
    return setup(q)[1]


def aa_pair(pos, tri, adj, rast, b, P, Q, axis):
    """the pair of pixels P = (x, y) and Q (its right / upper neighbour): None, or (near (0: P), t, e, alpha, dA (3,), dB (3,))
    with the partials of alpha by (x, y, w) of corners e and e + 1 of t, in the kernel's fp32 order"""
    H, W = rast.shape[1], rast.shape[2]
    idP, idQ = int(rast[b, P[1], P[0], 3]), int(rast[b, Q[1], Q[0], 3])
    if idP == idQ:
        return None
    zP = rast[b, P[1], P[0], 2] if idP else F32(np.inf)
    zQ = rast[b, Q[1], Q[0], 2] if idQ else F32(np.inf)
    near = 0 if zP <= zQ else 1
    t = (idQ if near else idP) - 1
    N = Q if near else P
    xn, yn = F32(N[0]) + F32(0.5), F32(N[1]) + F32(0.5)
    dirn = F32(-1.0) if near else F32(1.0)
    q = pos[b, tri[t]]
    st = _det(q) > 0.0
    hw, hh = F32(0.5) * F32(W), F32(0.5) * F32(H)
    for e in range(3):
        A, Bv = q[e], q[(e + 1) % 3]
        if not (A[3] > 0 and Bv[3] > 0):
            continue
        o = adj[t, e]
        if o >= 0 and (_det(pos[b, tri[o]]) > 0.0) == st:
            continue
        XA, YA = (A[0] / A[3] + F32(1.0)) * hw, (A[1] / A[3] + F32(1.0)) * hh
        XB, YB = (Bv[0] / Bv[3] + F32(1.0)) * hw, (Bv[1] / Bv[3] + F32(1.0)) * hh
        steep = abs(YB - YA) > abs(XB - XA)          # mostly vertical edges blend horizontal pairs, the others vertical pairs
        if steep == (axis == 1):
            continue
        alA, alB, acA, acB = (YA, YB, XA, XB) if axis else (XA, XB, YA, YB)
        line, start = (xn, yn) if axis else (yn, xn)
        if (acA < line) == (acB < line):
            continue
        d = acB - acA
        tt = (line - acA) / d
        hit = alA + tt * (alB - alA)
        alpha = (hit - start) * dirn
        if not (alpha >= 0 and alpha <= 1):
            continue
        d_alA, d_alB = dirn * (F32(1.0) - tt), dirn * tt
        d_acA, d_acB = dirn * (alB - alA) * (tt - F32(1.0)) / d, dirn * (alB - alA) * (-tt / d)
        dXA, dYA, dXB, dYB = (d_acA, d_alA, d_acB, d_alB) if axis else (d_alA, d_acA, d_alB, d_acB)
        dA = np.array([dXA * hw / A[3], dYA * hh / A[3], -(dXA * hw * A[0] + dYA * hh * A[1]) / (A[3] * A[3])], dtype=F32)
        dB = np.array([dXB * hw / Bv[3], dYB * hh / Bv[3], -(dXB * hw * Bv[0] + dYB * hh * Bv[1]) / (Bv[3] * Bv[3])], dtype=F32)
        return near, t, e, alpha, dA, dB
    return None


def _pairs(W, H, x, y):
    """the pairs of pixel (x, y) in the kernel's order: (P, Q, axis, self_is_P)"""
    if x > 0:
        yield (x - 1, y), (x, y), 0, False
    if x + 1 < W:
        yield (x, y), (x + 1, y), 0, True
    if y > 0:
        yield (x, y - 1), (x, y), 1, False
    if y + 1 < H:
        yield (x, y), (x, y + 1), 1, True


def _receiver(near, alpha, selfP):
    self_near = (near == 0) == selfP
    return (not self_near) if alpha > 0.5 else self_near


def antialias(color, rast, pos, tri):
    color = np.asarray(color, dtype=F32)
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    adj = adjacency(tri)
    B, H, W, C = color.shape
    out = color.copy()
    for b in range(B):
        for y in range(H):
            for x in range(W):
                for P, Q, axis, selfP in _pairs(W, H, x, y):
                    h = aa_pair(pos, tri, adj, rast, b, P, Q, axis)
                    if h is None or not _receiver(h[0], h[3], selfP):
                        continue
                    o = Q if selfP else P
                    alpha = h[3]
                    fac = alpha - F32(0.5) if alpha > 0.5 else F32(0.5) - alpha
                    out[b, y, x] = out[b, y, x] + fac * (color[b, o[1], o[0]] - color[b, y, x])
    return out


def antialias_backward(color, rast, pos, tri, g, boost=1.0):
    """(grad_color, grad_pos (B, V, 4), [..., 2] = 0) in fp64"""
    color = np.asarray(color, dtype=F32)
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    adj = adjacency(tri)
    B, H, W, C = color.shape
    gc = g.astype(np.float64).copy()
    gp = np.zeros(pos.shape, dtype=np.float64)
    for b in range(B):
        for y in range(H):
            for x in range(W - 1 + 1):
                for P, Q, axis, selfP in _pairs(W, H, x, y):
                    if not selfP:
                        continue                       # each pair once, from P
                    h = aa_pair(pos, tri, adj, rast, b, P, Q, axis)
                    if h is None:
                        continue
                    near, t, e, alpha, dA, dB = h
                    n_pix, o_pix = (Q, P) if near else (P, Q)
                    far_gets = alpha > 0.5
                    r, s = (o_pix, n_pix) if far_gets else (n_pix, o_pix)
                    fac = float(alpha) - 0.5 if far_gets else 0.5 - float(alpha)
                    gr = g[b, r[1], r[0]].astype(np.float64)
                    gc[b, r[1], r[0]] -= fac * gr
                    gc[b, s[1], s[0]] += fac * gr
                    dl = (gr * (color[b, s[1], s[0]].astype(np.float64) - color[b, r[1], r[0]])).sum()
                    dl = (dl if far_gets else -dl) * boost
                    gp[b, tri[t, e], [0, 1, 3]] += dl * dA
                    gp[b, tri[t, (e + 1) % 3], [0, 1, 3]] += dl * dB
    return gc, gp
