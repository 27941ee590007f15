"""
Vectorised restatement of tests/render_statement.py (which stays the specification): the same decisions and the same fp32 / fp64
operation order, evaluated over arrays of candidates, pixels or pixel pairs instead of Python loops, so that the device can be checked
at production shapes. tests/test_render_statement_cpu.py proves every function here equal to its loop version (id maps and fp32
outputs bitwise, fp64 gradients to 1e-12).

The backwards also return, per output element, the sum of the absolute values of its terms (`abs`), and `seg_depth` / `vertex_depth`
give the depth of the kernel's fp32 summation: with them a device gradient is checked element by element against
    |dev - ref| <= (depth + slack) * 2^-24 * abs
(see `bound` and tests/test_render_scale_gpu.py for the derivation of each slack).
"""
import numpy as np

import render_statement as rs

F32 = np.float32
F64 = np.float64
_NONE = np.iinfo(np.uint64).max
U = 2.0 ** -24                                  # unit roundoff of fp32


def setup(q):
    """q (n, 3, 4) fp32 -> c (n, 3, 3), D (n,): rs.setup over an array of triangles"""
    c = np.stack([rs._cross(q[:, 1], q[:, 2]), rs._cross(q[:, 2], q[:, 0]), rs._cross(q[:, 0], q[:, 1])], axis=1)
    D = (q[:, 0, 0].astype(F64) * c[:, 0, 0] + q[:, 0, 1].astype(F64) * c[:, 0, 1]) + q[:, 0, 3].astype(F64) * c[:, 0, 2]
    return c, D


def _edges(c, px, py):
    return [(px * c[:, i, 0] + py * c[:, i, 1]) + c[:, i, 2] for i in range(3)]


def cover(q, c, D, px, py):
    """rs.cover for candidate i = (triangle q[i] with setup c[i], D[i]; centre px[i], py[i]): (mask, E list, zf)"""
    s = np.where(D > 0.0, 1.0, -1.0)
    E = _edges(c, px, py)
    inside = np.ones(px.shape, dtype=bool)
    for i in range(3):
        e = s * E[i]
        cx, cy = s * c[:, i, 0], s * c[:, i, 1]
        inside &= (e > 0.0) | ((e == 0.0) & ((cx > 0.0) | ((cx == 0.0) & (cy > 0.0))))
    S = (E[0] + E[1]) + E[2]
    with np.errstate(all="ignore"):
        inside &= s * S > 0.0
        zw = ((q[:, 0, 2].astype(F64) * E[0] + q[:, 1, 2].astype(F64) * E[1]) + q[:, 2, 2].astype(F64) * E[2]) / D
        zf = zw.astype(F32)
    inside &= (zf >= F32(-1.0)) & (zf <= F32(1.0))
    inside &= (D != 0.0) & ~np.isnan(D)
    return inside, E, zf


def visible(q, D):
    """the kernel's rs_visible: False where the triangle can cover nothing"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    cull = ~(w > 0).any(1)
    for a in (x, y, z):
        cull |= (a > w).all(1) | (a < -w).all(1)
    return ~cull & (D != 0.0) & ~np.isnan(D)


def bbox(q, H, W):
    """the kernel's rs_bbox, one-pixel margin included, whole image when a corner has w <= 0: (x0, x1, y0, y1) int64, nonempty mask"""
    n = q.shape[0]
    front = (q[..., 3] > 0).all(1)
    with np.errstate(all="ignore"):
        X = q[..., 0].astype(F64) / q[..., 3].astype(F64)
        Y = q[..., 1].astype(F64) / q[..., 3].astype(F64)
    mnx = np.fmin(np.fmin(np.fmin(1e300, X[:, 0]), X[:, 1]), X[:, 2])
    mxx = np.fmax(np.fmax(np.fmax(-1e300, X[:, 0]), X[:, 1]), X[:, 2])
    mny = np.fmin(np.fmin(np.fmin(1e300, Y[:, 0]), Y[:, 1]), Y[:, 2])
    mxy = np.fmax(np.fmax(np.fmax(-1e300, Y[:, 0]), Y[:, 1]), Y[:, 2])
    with np.errstate(all="ignore"):
        ax = np.fmax(np.floor(((mnx + 1.0) * W - 1.0) * 0.5) - 1.0, 0.0)
        bx = np.fmin(np.ceil(((mxx + 1.0) * W - 1.0) * 0.5) + 1.0, W - 1.0)
        ay = np.fmax(np.floor(((mny + 1.0) * H - 1.0) * 0.5) - 1.0, 0.0)
        by = np.fmin(np.ceil(((mxy + 1.0) * H - 1.0) * 0.5) + 1.0, H - 1.0)
    ok = (ax <= bx) & (ay <= by)
    ax, bx, ay, by = (np.where(front, a, d) for a, d in ((ax, 0.0), (bx, W - 1.0), (ay, 0.0), (by, H - 1.0)))
    ok = np.where(front, ok, True)
    ax, bx, ay, by = (np.where(ok, a, 0).astype(np.int64) for a in (ax, bx, ay, by))
    return ax, bx, ay, by, ok & np.ones(n, dtype=bool)


def rasterize(pos, tri, H, W, chunk=1 << 21):
    """rs.rasterize: candidates (image, face, pixel of the face's box) in chunks of about `chunk`, per-pixel minimum of the 64-bit key"""
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    B = pos.shape[0]
    cw, ch = rs.centres(W), rs.centres(H)
    rast = np.zeros((B, H, W, 4), dtype=F32)
    for b in range(B):
        best = np.full(H * W, _NONE, dtype=np.uint64)
        q = pos[b][tri] if tri.shape[0] else np.zeros((0, 3, 4), F32)
        c, D = setup(q)
        x0, x1, y0, y1, ok = bbox(q, H, W)
        fs = np.nonzero(visible(q, D) & ok)[0]
        bw = x1[fs] - x0[fs] + 1
        n = bw * (y1[fs] - y0[fs] + 1)
        cum = np.cumsum(n)
        s = 0
        while s < len(fs):
            base = cum[s - 1] if s else 0
            e = max(int(np.searchsorted(cum, base + chunk, side="right")), s + 1)
            nn = n[s:e]
            k = np.repeat(np.arange(s, e), nn)
            j = np.arange(int(nn.sum()), dtype=np.int64) - np.repeat(cum[s:e] - nn - base, nn)
            xs = x0[fs[k]] + j % bw[k]
            ys = y0[fs[k]] + j // bw[k]
            f = fs[k]
            m, _, zf = cover(q[f], c[f], D[f], cw[xs], ch[ys])
            key = (rs._order_bits(zf[m]) << np.uint64(32)) | f[m].astype(np.uint64)
            np.minimum.at(best, ys[m] * W + xs[m], key)
            s = e
        hit = np.nonzero(best != _NONE)[0]
        f = (best[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        ys, xs = hit // W, hit % W
        _, E, zf = cover(q[f], c[f], D[f], cw[xs], ch[ys])
        S = (E[0] + E[1]) + E[2]
        out = rast[b].reshape(-1, 4)
        out[hit] = np.stack([(E[0] / S).astype(F32), (E[1] / S).astype(F32), zf, (f + 1).astype(F32)], axis=-1)
    return rast


def _covered(rast):
    """(b, y, x, face) of every covered pixel"""
    b, y, x = np.nonzero(rast[..., 3])
    return b, y, x, rast[b, y, x, 3].astype(np.int64) - 1


def rasterize_backward(pos, tri, rast, g_rast, chunk=1 << 21):
    """rs.rasterize_backward: (grad_pos (B, V, 4) fp64, abs (B, V, 4)); a term of corner j is m1 (q_{j+1} x p) + m2 (p x q_{j-1}) and
    its `abs` is |m1 (q_{j+1} x p)| + |m2 (p x q_{j-1})|, component by component"""
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    V = pos.shape[1]
    gp = np.zeros((B * V, 4), dtype=F64)
    ab = np.zeros((B * V, 4), dtype=F64)
    cw, ch = rs.centres(W), rs.centres(H)
    bb, yy, xx, ff = _covered(rast)
    for s in range(0, len(ff), chunk):
        b, y, x, f = bb[s:s + chunk], yy[s:s + chunk], xx[s:s + chunk], ff[s:s + chunk]
        q = pos[b[:, None], tri[f]]
        c, _ = setup(q)
        p = np.stack([cw[x], ch[y], np.ones(len(x))], axis=1)
        E = np.einsum("nij,nj->ni", c, p)
        S = E.sum(1)
        gu, gv = g_rast[b, y, x, 0].astype(F64), g_rast[b, y, x, 1].astype(F64)
        dot = gu * E[:, 0] / S + gv * E[:, 1] / S
        dE = np.stack([gu - dot, gv - dot, -dot], axis=1) / S[:, None]
        Q = q[:, :, [0, 1, 3]].astype(F64)
        for j in range(3):
            t1 = dE[:, (j + 2) % 3, None] * np.cross(Q[:, (j + 1) % 3], p)
            t2 = dE[:, (j + 1) % 3, None] * np.cross(p, Q[:, (j + 2) % 3])
            idx = b * V + tri[f, j]
            for k, comp in enumerate((0, 1, 3)):
                gp[:, comp] += np.bincount(idx, weights=t1[:, k] + t2[:, k], minlength=B * V)
                ab[:, comp] += np.bincount(idx, weights=np.abs(t1[:, k]) + np.abs(t2[:, k]), minlength=B * V)
    return gp.reshape(B, V, 4), ab.reshape(B, V, 4)


def interpolate(attr, rast, tri):
    """rs.interpolate (fp32, the same operation order)"""
    attr = np.asarray(attr, dtype=F32)
    if attr.ndim == 2:
        attr = attr[None]
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    out = np.zeros((B, H, W, attr.shape[2]), dtype=F32)
    b, y, x, f = _covered(rast)
    a = attr[0 if attr.shape[0] == 1 else b[:, None], tri[f]]            # (n, 3, C)
    u, v = rast[b, y, x, 0][:, None], rast[b, y, x, 1][:, None]
    w = (F32(1.0) - u) - v
    out[b, y, x] = (u * a[:, 0] + v * a[:, 1]) + w * a[:, 2]
    return out


def interpolate_backward(attr, rast, tri, g):
    """rs.interpolate_backward: (grad_attr like attr, grad_rast (B, H, W, 4), abs of grad_attr, abs of grad_rast), fp64.
    abs of a term: |u g|, |v g| and, for the third corner, |g| (|1 - u| + |v| + |w|) -- the kernel forms w = (1 - u) - v in fp32, whose
    two roundings are then within 2^-24 of that; abs of grad_rast: sum over channels of |g (a_i - a_2)|"""
    attr = np.asarray(attr, dtype=F32)
    shape = attr.shape
    a3 = attr[None] if attr.ndim == 2 else attr
    tri = np.asarray(tri, dtype=np.int64)
    Ba, V, C = a3.shape
    B, H, W, _ = rast.shape
    b, y, x, f = _covered(rast)
    bb = np.zeros_like(b) if Ba == 1 else b
    u, v = rast[b, y, x, 0].astype(F64), rast[b, y, x, 1].astype(F64)
    gg = g[b, y, x].astype(F64)                                            # (n, C)
    w64 = 1.0 - u - v
    w32 = ((F32(1.0) - rast[b, y, x, 0]) - rast[b, y, x, 1]).astype(F64)
    ga = np.zeros((Ba * V, C), dtype=F64)
    ab = np.zeros((Ba * V, C), dtype=F64)
    coef = (u, v, w64)
    acoef = (np.abs(u), np.abs(v), np.abs(1.0 - u) + np.abs(v) + np.abs(w32))
    for j in range(3):
        idx = bb * V + tri[f, j]
        for cc in range(C):
            ga[:, cc] += np.bincount(idx, weights=coef[j] * gg[:, cc], minlength=Ba * V)
            ab[:, cc] += np.bincount(idx, weights=acoef[j] * np.abs(gg[:, cc]), minlength=Ba * V)
    gr = np.zeros((B, H, W, 4), dtype=F64)
    ar = np.zeros((B, H, W, 4), dtype=F64)
    a = a3[bb[:, None], tri[f]]                                            # (n, 3, C) fp32
    for k in range(2):
        t = gg * (a[:, k] - a[:, 2])
        gr[b, y, x, k] = t.sum(1)
        ar[b, y, x, k] = np.abs(t).sum(1)
    return ga.reshape(shape), gr, ab.reshape(shape), ar


# ---- antialias --------------------------------------------------------------------------------------------------------------------
def adjacency(tri):
    """rs.adjacency by a sort of the half-edges: the face across edge (corner e, e + 1), -1 unless the edge has exactly two faces"""
    tri = np.asarray(tri, dtype=np.int64)
    F = tri.shape[0]
    a, b = tri, np.roll(tri, -1, axis=1)
    lo, hi = np.minimum(a, b).ravel(), np.maximum(a, b).ravel()
    h = np.lexsort((np.arange(3 * F), hi, lo))
    lo, hi = lo[h], hi[h]
    new = np.ones(3 * F + 1, dtype=bool)
    new[1:-1] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    start = np.nonzero(new)[0]
    cnt = np.diff(start)
    two = start[:-1][cnt == 2]
    adj = -np.ones(3 * F, dtype=np.int64)
    adj[h[two]], adj[h[two + 1]] = h[two + 1] // 3, h[two] // 3
    return adj.reshape(F, 3)


def aa_pairs(pos, tri, adj, rast, b, axis):
    """rs.aa_pair for every pair of image b along `axis` (0: (x, y)-(x + 1, y), shape (H, W - 1); 1: (x, y)-(x, y + 1), (H - 1, W)):
    dict of arrays found, near, t, e, alpha, dA (..., 3), dB (..., 3), in the kernel's fp32 order"""
    H, W = rast.shape[1], rast.shape[2]
    r = rast[b]
    P = r[:, :-1] if axis == 0 else r[:-1, :]
    Q = r[:, 1:] if axis == 0 else r[1:, :]
    shape = P.shape[:2]
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    idP, idQ = P[..., 3].astype(np.int64), Q[..., 3].astype(np.int64)
    cand = idP != idQ
    inf = F32(np.inf)
    zP = np.where(idP != 0, P[..., 2], inf)
    zQ = np.where(idQ != 0, Q[..., 2], inf)
    near = np.where(zP <= zQ, 0, 1)
    t = np.where(near == 1, idQ, idP) - 1
    xn = (xx + (near if axis == 0 else 0)).astype(F32) + F32(0.5)
    yn = (yy + (near if axis == 1 else 0)).astype(F32) + F32(0.5)
    dirn = np.where(near == 1, F32(-1.0), F32(1.0)).astype(F32)
    pb = pos[b]
    Dface = setup(pb[tri])[1] if tri.shape[0] else np.zeros(0)
    tt_ = np.where(cand, t, 0)
    st = Dface[tt_] > 0.0 if tri.shape[0] else np.zeros(shape, bool)
    hw, hh = F32(0.5) * F32(W), F32(0.5) * F32(H)
    found = np.zeros(shape, dtype=bool)
    out_e = np.zeros(shape, dtype=np.int64)
    alpha_o = np.zeros(shape, dtype=F32)
    dA_o = np.zeros(shape + (3,), dtype=F32)
    dB_o = np.zeros(shape + (3,), dtype=F32)
    if tri.shape[0] == 0:
        return dict(found=found, near=near, t=t, e=out_e, alpha=alpha_o, dA=dA_o, dB=dB_o)
    with np.errstate(all="ignore"):
        for e in range(3):
            A = pb[tri[tt_, e]]
            Bv = pb[tri[tt_, (e + 1) % 3]]
            ok = cand & ~found & (A[..., 3] > 0) & (Bv[..., 3] > 0)
            o = adj[tt_, e]
            ok &= (o < 0) | ((Dface[np.where(o >= 0, o, 0)] > 0.0) != st)
            XA, YA = (A[..., 0] / A[..., 3] + F32(1.0)) * hw, (A[..., 1] / A[..., 3] + F32(1.0)) * hh
            XB, YB = (Bv[..., 0] / Bv[..., 3] + F32(1.0)) * hw, (Bv[..., 1] / Bv[..., 3] + F32(1.0)) * hh
            steep = np.abs(YB - YA) > np.abs(XB - XA)
            ok &= steep != (axis == 1)
            alA, alB, acA, acB = (YA, YB, XA, XB) if axis else (XA, XB, YA, YB)
            line, start = (xn, yn) if axis else (yn, xn)
            ok &= (acA < line) != (acB < line)
            d = acB - acA
            tt = (line - acA) / d
            hit = alA + tt * (alB - alA)
            alpha = (hit - start) * dirn
            ok &= (alpha >= 0) & (alpha <= 1)
            d_alA, d_alB = dirn * (F32(1.0) - tt), dirn * tt
            d_acA, d_acB = dirn * (alB - alA) * (tt - F32(1.0)) / d, dirn * (alB - alA) * (-tt / d)
            dXA, dYA, dXB, dYB = (d_acA, d_alA, d_acB, d_alB) if axis else (d_alA, d_acA, d_alB, d_acB)
            dA = np.stack([dXA * hw / A[..., 3], dYA * hh / A[..., 3], -(dXA * hw * A[..., 0] + dYA * hh * A[..., 1]) / (A[..., 3] * A[..., 3])], -1)
            dB = np.stack([dXB * hw / Bv[..., 3], dYB * hh / Bv[..., 3],
                           -(dXB * hw * Bv[..., 0] + dYB * hh * Bv[..., 1]) / (Bv[..., 3] * Bv[..., 3])], -1)
            out_e[ok], alpha_o[ok], dA_o[ok], dB_o[ok] = e, alpha[ok], dA[ok], dB[ok]
            found |= ok
    return dict(found=found, near=near, t=t, e=out_e, alpha=alpha_o, dA=dA_o, dB=dB_o)


def _directions(H, W):
    """the kernel's pair order of a pixel (left, right, below, above): (axis, selfP, slice of the pixel grid, slice of the pair grid,
    offset of the other pixel)"""
    return [(0, False, np.s_[:, 1:], np.s_[:, :], (0, -1)), (0, True, np.s_[:, :-1], np.s_[:, :], (0, 1)),
            (1, False, np.s_[1:, :], np.s_[:, :], (-1, 0)), (1, True, np.s_[:-1, :], np.s_[:, :], (1, 0))]


def _shift(a, off):
    dy, dx = off
    H, W = a.shape[:2]
    return a[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]


def antialias(color, rast, pos, tri, adj=None):
    """rs.antialias (fp32, the same per-pixel order of pairs)"""
    color = np.asarray(color, dtype=F32)
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    adj = adjacency(tri) if adj is None else adj
    B, H, W, C = color.shape
    out = color.copy()
    for b in range(B):
        pr = [aa_pairs(pos, tri, adj, rast, b, a) if (W > 1 if a == 0 else H > 1) else None for a in (0, 1)]
        for axis, selfP, sl, _, off in _directions(H, W):
            h = pr[axis]
            if h is None:
                continue
            self_near = (h["near"] == 0) == selfP
            recv = h["found"] & np.where(h["alpha"] > F32(0.5), ~self_near, self_near)
            fac = np.where(h["alpha"] > F32(0.5), h["alpha"] - F32(0.5), F32(0.5) - h["alpha"])
            o = out[b][sl]
            cs = color[b][sl]
            co = _shift(color[b], off)
            o[recv] = o[recv] + fac[recv][:, None] * (co[recv] - cs[recv])
    return out


def antialias_backward(color, rast, pos, tri, g, boost=1.0, adj=None):
    """rs.antialias_backward: (grad_color, grad_pos (B, V, 4), abs of grad_color, abs of grad_pos, terms of grad_color, pos_terms) in
    fp64. A position term is dl * dA_q with dl = boost * sum_c g_c (c_s - c_r); its abs is |boost| sum_c |g_c (c_s - c_r)| |dA_q|.
    pos_terms (B, F) counts the (pixel, pair) terms of each face's row."""
    color = np.asarray(color, dtype=F32)
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    adj = adjacency(tri) if adj is None else adj
    B, H, W, C = color.shape
    V, F = pos.shape[1], tri.shape[0]
    gc = g.astype(F64).copy()
    agc = np.abs(gc)
    ngc = np.ones((B, H, W), dtype=np.int64)
    gp = np.zeros((B * V, 4), dtype=F64)
    agp = np.zeros((B * V, 4), dtype=F64)
    nterm = np.zeros((B, F), dtype=np.int64)
    for b in range(B):
        for axis in (0, 1):
            if (W if axis == 0 else H) < 2:
                continue
            h = aa_pairs(pos, tri, adj, rast, b, axis)
            py, px = np.nonzero(h["found"])
            qy, qx = (py, px + 1) if axis == 0 else (py + 1, px)
            near = h["near"][py, px]
            alpha = h["alpha"][py, px]
            ny, nx = np.where(near == 1, qy, py), np.where(near == 1, qx, px)
            oy, ox = np.where(near == 1, py, qy), np.where(near == 1, px, qx)
            far_gets = alpha > F32(0.5)
            ry, rx = np.where(far_gets, oy, ny), np.where(far_gets, ox, nx)
            sy, sx = np.where(far_gets, ny, oy), np.where(far_gets, nx, ox)
            fac = np.where(far_gets, alpha.astype(F64) - 0.5, 0.5 - alpha.astype(F64))
            gr = g[b, ry, rx].astype(F64)
            np.add.at(gc[b], (ry, rx), -fac[:, None] * gr)
            np.add.at(gc[b], (sy, sx), fac[:, None] * gr)
            np.add.at(agc[b], (ry, rx), np.abs(fac[:, None] * gr))
            np.add.at(agc[b], (sy, sx), np.abs(fac[:, None] * gr))
            np.add.at(ngc[b], (ry, rx), 1)
            np.add.at(ngc[b], (sy, sx), 1)
            prod = gr * (color[b, sy, sx].astype(F64) - color[b, ry, rx])
            dl = np.where(far_gets, 1.0, -1.0) * prod.sum(1) * boost
            adl = np.abs(prod).sum(1) * abs(boost)
            t, e = h["t"][py, px], h["e"][py, px]
            np.add.at(nterm[b], t, 1)
            for corner, dd in ((tri[t, e], h["dA"][py, px]), (tri[t, (e + 1) % 3], h["dB"][py, px])):
                idx = b * V + corner
                for k, comp in enumerate((0, 1, 3)):
                    gp[:, comp] += np.bincount(idx, weights=dl * dd[:, k], minlength=B * V)
                    agp[:, comp] += np.bincount(idx, weights=adl * np.abs(dd[:, k].astype(F64)), minlength=B * V)
    return gc, gp.reshape(B, V, 4), agc, agp.reshape(B, V, 4), ngc, nterm


# ---- the kernels' summation depth --------------------------------------------------------------------------------------------------
def face_pixels(rast, F):
    """(B, F) pixel count of every (image, face): the length m of its segment in the pixel order"""
    B = rast.shape[0]
    m = np.zeros((B, F), dtype=np.int64)
    for b in range(B):
        ids = rast[b, ..., 3].astype(np.int64).ravel()
        m[b] = np.bincount(ids[ids > 0] - 1, minlength=F)[:F]
    return m


def seg_depth(m, terms=None):
    """depth of k_rs_seg_sum's fp32 sum of a face row over its m pixels: one thread adds the terms in order (m of them, or `terms`
    when a pixel adds several); a face of more than 64 pixels is summed lane-strided (ceil(m / 64) pixels a lane) and then by a 6-level
    butterfly"""
    per_pixel = 1 if terms is None else 4
    n = m if terms is None else terms
    wave = np.minimum(n, per_pixel * ((m + 63) // 64)) + 6
    return np.where(m > 64, wave, n)


def vertex_depth(dface, tri, V, batches_summed=False):
    """per (image, vertex) (or per vertex, batches_summed): the largest face depth among its corners plus the length of the per-vertex
    chain (k_rs_gather_pos: its corner count; k_rs_gather_attr with one attribute batch: B times its corner count)"""
    tri = np.asarray(tri, dtype=np.int64)
    B = dface.shape[0]
    k = np.bincount(tri.ravel(), minlength=V)[:V]
    d = np.zeros((B, V), dtype=np.int64)
    for b in range(B):
        np.maximum.at(d[b], tri.ravel(), np.repeat(dface[b], 3))
    if batches_summed:
        return d.max(0) + B * k
    return d + k[None]


def bound(depth, ab, slack):
    return (depth + slack) * U * ab
