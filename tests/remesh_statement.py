"""
Numpy statement of the Botsch-Kobbelt remesher of csrc/remesh.hip (largesteps.remesh.remesh_botsch): the executable contract.

Every decision rule, tie-break and fp32 operation order below is the kernel's ("Isotropic remeshing"). The kernel and this
statement must produce identical face arrays and positions within 2 ulp; the projection is a brute-force fp64 closest point here and
a BVH query with the same fp64 point-triangle test on the device (same result: the minimum of (distance^2, triangle id)).

Layout: verts (V, 3) float32, faces (F, 3) int64 here (int32 on the device). Half-edge h = 3 f + k runs from faces[f, k] to
faces[f, (k + 1) % 3]; twin[h] is the opposite half-edge or -1 (boundary). The edge of h is identified by min(h, twin[h]) (h itself on
the boundary): its "edge id".
"""
import numpy as np

F32 = np.float32
SPLIT_ROUNDS, COLLAPSE_ROUNDS, FLIP_ROUNDS = 8, 64, 64        # round caps of one phase (the kernel's)


class MeshError(ValueError):
    pass


# ---- topology ---------------------------------------------------------------------------------------------------------------
class Topo:
    """tables of one round: twin, per-vertex corners (ascending corner id), corner counts, boundary flags, valences"""

    def __init__(self, V, F):
        F = np.asarray(F, dtype=np.int64)
        nV, nF = V.shape[0], F.shape[0]
        self.F, self.nV = F, nV
        org = F.reshape(-1)
        dst = F[:, [1, 2, 0]].reshape(-1)
        self.org, self.dst = org, dst
        key = org * nV + dst
        order = np.argsort(key, kind="stable")
        sk = key[order]
        rkey = dst * nV + org
        pos = np.searchsorted(sk, rkey)
        pos_c = np.minimum(pos, sk.size - 1)
        found = (pos < sk.size) & (sk[pos_c] == rkey)
        self.twin = np.where(found, order[pos_c], -1)
        self.vorder = np.argsort(org, kind="stable")                 # corners grouped by vertex, ascending corner id
        self.cnt = np.bincount(org, minlength=nV)
        self.vptr = np.concatenate([[0], np.cumsum(self.cnt)])
        self.bnd = np.zeros(nV, dtype=bool)
        self.bnd[org[self.twin < 0]] = True
        self.val = self.cnt + self.bnd.astype(np.int64)
        self.eid = np.where(self.twin < 0, np.arange(3 * nF), np.minimum(np.arange(3 * nF), self.twin))

    def ring(self):
        """(V, maxdeg) padded corner table (-1 past a vertex's corner count), ascending corner id"""
        deg = self.cnt
        W = int(deg.max(initial=0))
        tab = -np.ones((self.nV, max(W, 1)), dtype=np.int64)
        slot = np.arange(self.vorder.size) - self.vptr[self.F.reshape(-1)[self.vorder]]
        tab[self.F.reshape(-1)[self.vorder], slot] = self.vorder
        return tab


def validate(V, F):
    """ValueError unless the mesh is an edge-manifold, consistently oriented triangle mesh whose vertices' faces form one fan each"""
    V = np.asarray(V)
    F = np.asarray(F, dtype=np.int64)
    if F.ndim != 2 or F.shape[1] != 3 or V.ndim != 2 or V.shape[1] != 3:
        raise MeshError("remesh_botsch: verts must be (n, 3) and faces (m, 3)")
    if F.size and (F.min() < 0 or F.max() >= V.shape[0]):
        raise MeshError("remesh_botsch: a face index is out of range")
    if np.any((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 2] == F[:, 0])):
        raise MeshError("remesh_botsch: a face repeats a vertex")
    nV = V.shape[0]
    org = F.reshape(-1)
    dst = F[:, [1, 2, 0]].reshape(-1)
    key = org * nV + dst
    if np.unique(key).size != key.size:
        raise MeshError("remesh_botsch: an edge is traversed twice in the same direction (non-manifold or inconsistently oriented)")
    t = Topo(V, F)
    nb_out = np.bincount(org[t.twin < 0], minlength=nV)
    if np.any(nb_out > 1):
        raise MeshError("remesh_botsch: the faces around a vertex form more than one fan")
    # walk each vertex's fan from its first corner (or its boundary corner): next corner = twin(prev(c))
    start = np.full(nV, -1, dtype=np.int64)
    used = t.cnt > 0
    start[used] = t.vorder[t.vptr[:-1][used]]                         # first corner of each vertex
    bc = np.nonzero(t.twin < 0)[0]
    start[org[bc]] = bc
    cur = start[used]
    steps = np.zeros(cur.size, dtype=np.int64)
    alive = np.ones(cur.size, dtype=bool)
    first = cur.copy()
    for _ in range(int(t.cnt.max(initial=0)) + 1):
        steps += alive
        prev = 3 * (cur // 3) + (cur + 2) % 3
        nxt = t.twin[prev]
        stop = alive & ((nxt < 0) | (nxt == first))
        alive &= ~stop
        cur = np.where(alive, nxt, cur)
    if np.any(alive) or np.any(steps != t.cnt[used]):
        raise MeshError("remesh_botsch: the faces around a vertex form more than one fan")


def drop_unreferenced(V, F):
    used = np.zeros(V.shape[0], dtype=bool)
    used[np.asarray(F).reshape(-1)] = True
    new = np.cumsum(used) - 1
    return V[used], new[F]


# ---- fp32 helpers (the kernel's operation order) -------------------------------------------------------------------------------
def len2(P, a, b):
    d = P[b] - P[a]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def mid(P, a, b):
    return (P[a] + P[b]) * F32(0.5)


def tri_normal(p0, p1, p2):
    e1, e2 = p1 - p0, p2 - p0
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def thresholds(h):
    h = F32(h)
    hi, lo = F32(F32(4.0) / F32(3.0)) * h, F32(F32(4.0) / F32(5.0)) * h
    return hi * hi, lo * lo


def _compact(V, F, keep_face, removed_vert):
    F = F[keep_face]
    alive = ~removed_vert
    new = np.cumsum(alive) - 1
    return V[alive], new[F]


# ---- phases: one round each; they return (verts, faces, count of operations) ----------------------------------------------------
def split_round(V, F, h):
    hi2, _ = thresholds(h)
    t = Topo(V, F)
    H = np.arange(3 * F.shape[0])
    canon = (t.twin >= 0) & (H < t.twin)
    L = len2(V, t.org, t.dst)
    # a face with a locked (boundary) edge longer than hi keeps its interior edges: splitting them would only cut slivers off it
    held = ((t.twin < 0) & (L > hi2)).reshape(-1, 3).any(axis=1)
    marked = canon & (L > hi2) & ~held[H // 3] & ~held[np.maximum(t.twin, 0) // 3]
    n = int(marked.sum())
    if n == 0:
        return V, F, 0
    nV = V.shape[0]
    mo = np.full(H.size, -1, dtype=np.int64)
    mo[marked] = nV + np.arange(n)                                    # midpoint ids: an exclusive scan of the marks over edge ids
    mid_of = np.where(canon, mo, np.where(t.twin >= 0, mo[np.maximum(t.twin, 0)], -1))
    Vn = np.concatenate([V, mid(V, t.org[marked], t.dst[marked])]).astype(F32)
    m = mid_of.reshape(-1, 3)
    out = []
    for f in range(F.shape[0]):
        out.extend(split_face(Vn, F[f], m[f]))
    return Vn, np.asarray(out, dtype=np.int64).reshape(-1, 3), n


def split_face(P, v, m):
    """1 + (marked edges) faces replacing face v (corners v[0..2], m[k] = midpoint of edge k = v[k] -> v[k + 1] or -1)"""
    mk = [k for k in range(3) if m[k] >= 0]
    if len(mk) == 0:
        return [tuple(v)]
    if len(mk) == 3:
        return [(v[0], m[0], m[2]), (m[0], v[1], m[1]), (m[2], m[1], v[2]), (m[0], m[1], m[2])]
    if len(mk) == 1:
        k = mk[0]
        a, b, c = v[k], v[(k + 1) % 3], v[(k + 2) % 3]
        return [(a, m[k], c), (m[k], b, c)]
    k = [j for j in range(3) if m[j] < 0][0]              # the unmarked edge a -> b; c the opposite corner
    a, b, c = v[k], v[(k + 1) % 3], v[(k + 2) % 3]
    mb, mc = m[(k + 1) % 3], m[(k + 2) % 3]               # midpoints of b -> c and c -> a
    # m = 2 rule: the quad (a, b, mb, mc) takes its shorter diagonal, a-mb on a tie
    da = len2(P, np.array([a]), np.array([mb]))[0]
    db = len2(P, np.array([b]), np.array([mc]))[0]
    if da <= db:
        return [(mc, mb, c), (a, b, mb), (a, mb, mc)]
    return [(mc, mb, c), (a, b, mc), (b, mb, mc)]


def _ring_min(t, m1):
    """m2[v] = min of m1 over v and its edge neighbours"""
    m2 = m1.copy()
    np.minimum.at(m2, t.dst, m1[t.org])
    np.minimum.at(m2, t.org, m1[t.dst])
    return m2


INF_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def collapse_round(V, F, h):
    hi2, lo2 = thresholds(h)
    t = Topo(V, F)
    nF = F.shape[0]
    H = np.arange(3 * nF)
    canon = (t.twin >= 0) & (H < t.twin)
    a, b = t.org, t.dst
    L = len2(V, a, b)
    cand = canon & ~t.bnd[a] & ~t.bnd[b] & (L < lo2)
    ring = t.ring()
    nbr = np.where(ring >= 0, t.dst[np.maximum(ring, 0)], -1)     # interior vertices: neighbours = destinations of the corners
    ok = np.zeros(H.size, dtype=bool)
    for e in np.nonzero(cand)[0]:
        ok[e] = collapse_ok(V, F, t, nbr, int(e), hi2)
    key = np.full(H.size, INF_KEY, dtype=np.uint64)
    key[ok] = (L[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | H[ok].astype(np.uint64)
    m1 = np.full(V.shape[0], INF_KEY, dtype=np.uint64)
    np.minimum.at(m1, a[ok], key[ok])
    np.minimum.at(m1, b[ok], key[ok])
    m3 = _ring_min(t, _ring_min(t, m1))
    win = ok & (key == m3[a]) & (key == m3[b])
    n = int(win.sum())
    if n == 0:
        return V, F, 0
    V = V.copy()
    ws = np.nonzero(win)[0]
    keep = np.minimum(a[ws], b[ws])
    gone = np.maximum(a[ws], b[ws])
    V[keep] = mid(V, a[ws], b[ws])
    remap = np.arange(V.shape[0])
    remap[gone] = keep
    keep_face = np.ones(nF, dtype=bool)
    keep_face[ws // 3] = False
    keep_face[t.twin[ws] // 3] = False
    removed = np.zeros(V.shape[0], dtype=bool)
    removed[gone] = True
    return (*_compact(V, remap[F], keep_face, removed), n)


def collapse_ok(V, F, t, nbr, e, hi2):
    a, b = int(t.org[e]), int(t.dst[e])
    Na = nbr[a][nbr[a] >= 0]
    Nb = nbr[b][nbr[b] >= 0]
    if t.val[a] < 4 or t.val[b] < 4:
        return False
    common = np.intersect1d(Na, Nb)
    if common.size != 2:
        return False
    if np.any(t.val[common] - 1 < 3):
        return False
    p = mid(V, np.array([a]), np.array([b]))
    # the union in corner order of a then b (the kernel's order; only a yes/no answer depends on it)
    for w in np.concatenate([Na, Nb]):
        if w == a or w == b:
            continue
        d = V[w] - p[0]
        if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > hi2:
            return False
    for v in (a, b):
        for c in t.vorder[t.vptr[v]:t.vptr[v + 1]]:
            f = c // 3
            fv = F[f]
            if (fv == a).any() and (fv == b).any():
                continue
            P = V[fv]
            Q = P.copy()
            Q[c % 3] = p[0]
            n0 = tri_normal(P[0:1], P[1:2], P[2:3])
            n1 = tri_normal(Q[0:1], Q[1:2], Q[2:3])
            if dot3(n0, n1)[0] <= F32(0):
                return False
    return True


def _target(t, v):
    return np.where(t.bnd[v], 4, 6)


def flip_round(V, F, h=None):
    t = Topo(V, F)
    nF = F.shape[0]
    H = np.arange(3 * nF)
    canon = (t.twin >= 0) & (H < t.twin)
    es = np.nonzero(canon)[0]
    a, b = t.org[es], t.dst[es]
    tw = t.twin[es]
    c = F.reshape(-1)[3 * (es // 3) + (es + 2) % 3]
    d = F.reshape(-1)[3 * (tw // 3) + (tw + 2) % 3]
    va, vb, vc, vd = t.val[a], t.val[b], t.val[c], t.val[d]
    before = (np.abs(va - _target(t, a)) + np.abs(vb - _target(t, b))) + (np.abs(vc - _target(t, c)) + np.abs(vd - _target(t, d)))
    after = (np.abs(va - 1 - _target(t, a)) + np.abs(vb - 1 - _target(t, b))) + (np.abs(vc + 1 - _target(t, c)) + np.abs(vd + 1 - _target(t, d)))
    gain = before - after
    ok = (gain > 0) & (va - 1 >= 3) & (vb - 1 >= 3) & (c != d)
    # c-d must not be an edge yet
    ekeys = set((t.org * t.nV + t.dst).tolist())
    for i in np.nonzero(ok)[0]:
        if int(c[i]) * t.nV + int(d[i]) in ekeys or int(d[i]) * t.nV + int(c[i]) in ekeys:
            ok[i] = False
    Fo = F[es // 3]
    Go = F[tw // 3]
    nf = tri_normal(V[Fo[:, 0]], V[Fo[:, 1]], V[Fo[:, 2]])
    ng = tri_normal(V[Go[:, 0]], V[Go[:, 1]], V[Go[:, 2]])
    n1 = tri_normal(V[c], V[a], V[d])
    n2 = tri_normal(V[d], V[b], V[c])
    for x in (n1, n2):
        for y in (nf, ng):
            ok &= dot3(x, y) > F32(0)
    key = np.full(es.size, INF_KEY, dtype=np.uint64)
    key[ok] = ((4 - gain[ok]).astype(np.uint64) << np.uint64(32)) | es[ok].astype(np.uint64)
    m = np.full(V.shape[0], INF_KEY, dtype=np.uint64)
    for x in (a, b, c, d):
        np.minimum.at(m, x[ok], key[ok])
    win = ok & (key == m[a]) & (key == m[b]) & (key == m[c]) & (key == m[d])
    n = int(win.sum())
    if n == 0:
        return V, F, 0
    F = F.copy()
    F[es[win] // 3] = np.stack([c[win], a[win], d[win]], axis=1)
    F[tw[win] // 3] = np.stack([d[win], b[win], c[win]], axis=1)
    return V, F, n


def relax(V, F, h=None):
    t = Topo(V, F)
    ring = t.ring()
    P = V
    q = np.zeros_like(P)
    n = np.zeros_like(P)
    Fl = F.reshape(-1)
    for j in range(ring.shape[1]):
        c = ring[:, j]
        has = c >= 0
        cc = np.maximum(c, 0)
        q = np.where(has[:, None], q + P[t.dst[cc]], q)
        f = cc // 3
        nf = tri_normal(P[Fl[3 * f]], P[Fl[3 * f + 1]], P[Fl[3 * f + 2]])
        n = np.where(has[:, None], n + nf, n)
    deg = t.cnt.astype(F32)
    move = (~t.bnd) & (t.cnt > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = q / deg[:, None]
        nl = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        u = n / nl[:, None]
        r = P - q
        s = (u[:, 0] * r[:, 0] + u[:, 1] * r[:, 1]) + u[:, 2] * r[:, 2]
        out = q + s[:, None] * u
    out = np.where((nl > F32(0))[:, None], out, q)
    return np.where(move[:, None], out, P).astype(F32), F, int(move.sum())


# ---- projection: brute-force fp64 closest point on the input mesh --------------------------------------------------------------
def _d(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_points(P, V0, F0):
    """(P.shape) closest points of P (fp64) on triangles V0[F0] (fp64): the region tests in the kernel's order; ties of the squared
    distance go to the lower triangle id"""
    P = P.astype(np.float64)
    A, B, C = (V0[F0[:, k]].astype(np.float64) for k in range(3))
    out = np.empty_like(P)
    for s in range(0, P.shape[0], 256):
        p = P[s:s + 256, None, :]
        q = point_triangle(p, A[None], B[None], C[None])
        dd = p - q
        d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        j = np.argmin(d2, axis=1)                    # first minimum = lowest triangle id
        out[s:s + 256] = q[np.arange(j.size), j]
    return out


def point_triangle(p, a, b, c):
    with np.errstate(divide="ignore", invalid="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _d(ab, ap), _d(ac, ap)
        bp = p - b
        d3, d4 = _d(ab, bp), _d(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _d(ab, cp), _d(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        r = (a + ab * v[..., None]) + ac * w[..., None]
        r = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * w_bc[..., None], r)
        r = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * w_ac[..., None], r)
        r = np.where(((d6 >= 0) & (d5 <= d6))[..., None], np.broadcast_to(c, r.shape), r)
        r = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * v_ab[..., None], r)
        r = np.where(((d3 >= 0) & (d4 <= d3))[..., None], np.broadcast_to(b, r.shape), r)
        r = np.where(((d1 <= 0) & (d2 <= 0))[..., None], np.broadcast_to(a, r.shape), r)
    return r


def _dt(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def point_triangle_torch(p, a, b, c):
    """point_triangle in torch, fp64 on any device: the same operations in the same order, so the same bits as numpy"""
    import torch
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dt(ab, ap), _dt(ac, ap)
    bp = p - b
    d3, d4 = _dt(ab, bp), _dt(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = p - c
    d5, d6 = _dt(ab, cp), _dt(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    v_ab = d1 / (d1 - d3)
    w_ac = d2 / (d2 - d6)
    w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = torch.ones_like(va) / ((va + vb) + vc)
    v, w = vb * den, vc * den
    r = (a + ab * v[..., None]) + ac * w[..., None]
    r = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * w_bc[..., None], r)
    r = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * w_ac[..., None], r)
    r = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c, r)
    r = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * v_ab[..., None], r)
    r = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b, r)
    r = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a, r)
    return r


def closest_points_torch(P, V0, F0, device="cpu", pchunk=1024, tchunk=4096):
    """closest_points on a torch device, in chunks of points and triangles: (closest points (n, 3), their squared distances (n,)),
    fp64 tensors on `device`. Same bits as closest_points: its region tests and order, and the first minimum over all triangles (a
    later chunk replaces the running best only when strictly closer; a NaN distance counts as the smallest, as in np.argmin)."""
    import torch

    def f64(x):
        return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(device=device, dtype=torch.float64)

    P, V0 = f64(P), f64(V0)
    F0 = (F0 if isinstance(F0, torch.Tensor) else torch.from_numpy(np.asarray(F0, dtype=np.int64))).to(device=device, dtype=torch.int64)
    A, B, C = (V0[F0[:, k]] for k in range(3))
    T = F0.shape[0]
    q_out = torch.empty_like(P)
    d_out = torch.empty(P.shape[0], dtype=torch.float64, device=device)
    for s in range(0, P.shape[0], pchunk):
        p = P[s:s + pchunk, None, :]
        rows = torch.arange(p.shape[0], device=device)
        best_k = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=device)
        best_q = p[:, 0, :].clone()
        best_d = best_k.clone()
        for t in range(0, T, tchunk):
            q = point_triangle_torch(p, A[None, t:t + tchunk], B[None, t:t + tchunk], C[None, t:t + tchunk])
            dd = p - q
            d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
            k = torch.where(torch.isnan(d2), float("-inf"), d2)
            m = k.min(dim=1).values
            ids = torch.arange(k.shape[1], device=device)
            j = torch.where(k == m[:, None], ids, k.shape[1]).min(dim=1).values           # first minimum of the chunk
            better = m < best_k
            best_k = torch.where(better, m, best_k)
            best_d = torch.where(better, d2[rows, j], best_d)
            best_q = torch.where(better[:, None], q[rows, j], best_q)
        q_out[s:s + pchunk] = best_q
        d_out[s:s + pchunk] = best_d
    return q_out, d_out


def closest_on(device, **chunks):
    """a `closest=` argument for project / iteration / remesh_botsch: closest_points computed by closest_points_torch on `device`"""
    def closest(P, V0, F0):
        return closest_points_torch(P, V0, F0, device, **chunks)[0].cpu().numpy()
    return closest


def project(V, F, V0, F0, closest=closest_points):
    t = Topo(V, F)
    move = (~t.bnd) & (t.cnt > 0)
    out = V.copy()
    if move.any():
        out[move] = closest(V[move], V0, F0).astype(F32)
    return out, F, int(move.sum())


# ---- a phase to fixpoint, one iteration, the full call --------------------------------------------------------------------------
def run_phase(fn, cap, V, F, h):
    rounds, ops = 0, 0
    while rounds < cap:
        V, F, n = fn(V, F, h)
        rounds += 1
        ops += n
        if n == 0:
            break
    return V, F, rounds, ops


def iteration(V, F, h, project_to=None, closest=closest_points, stats=None):
    """one iteration; `stats` (a dict, optional) accumulates the rounds and operations of each phase (the device's info() counters)"""
    for name, fn, cap in (("split", split_round, SPLIT_ROUNDS), ("collapse", collapse_round, COLLAPSE_ROUNDS), ("flip", flip_round, FLIP_ROUNDS)):
        V, F, rounds, ops = run_phase(fn, cap, V, F, h)
        if stats is not None:
            stats.setdefault("rounds", {}).setdefault(name, 0)
            stats.setdefault("ops", {}).setdefault(name, 0)
            stats["rounds"][name] += rounds
            stats["ops"][name] += ops
    V, F, _ = relax(V, F)
    if project_to is not None:
        V, F, _ = project(V, F, *project_to, closest=closest)
    return V, F


def remesh_botsch(V, F, iters, h, project=True, closest=closest_points, stats=None):
    V = np.asarray(V, dtype=F32)
    F = np.asarray(F, dtype=np.int64)
    validate(V, F)
    V, F = drop_unreferenced(V, F)
    V0, F0 = V.copy(), F.copy()
    if stats is not None:
        for k in ("rounds", "ops"):
            stats.setdefault(k, {}).update({name: stats.get(k, {}).get(name, 0) for name in ("split", "collapse", "flip")})
    for _ in range(iters):
        V, F = iteration(V, F, h, (V0, F0) if project else None, closest, stats)
    return V, F
