"""
The rule of csrc/winding.hip in numpy fp64: the solid angle of a face, the exact winding number, the node
moments of a hierarchy from their definitions (a sum per node, no bottom-up pass and no re-centring), and the walk. The hierarchy is
a dict in the device's format -- left, right (T - 1), esc (2 T - 1), tri (T), box (2 T - 1, 6) fp32, plus the mesh V (fp32) and F --
internal node i of T - 1, leaf i at T - 1 + i holding face tri[i]; `build_tree` makes one on the host (a median split, so the CPU
tests need no device), the GPU tests export the device's own.

Moments are (2 T - 1, 36) fp64 rows: p (3), r, N (3), Ar, C (9: row i column j at 3 i + j), T (18: row i at 6 i, columns jk = 00 01
02 11 12 22), one pad.
"""
import numpy as np

STRIDE = 36
P_, R_, N_, AR_, C_, T_ = 0, 3, 4, 7, 8, 17
SYM = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
FOUR_PI = 4.0 * np.pi


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _face_terms(q, a, b, c):
    """Omega / 4 pi of the faces (a, b, c) seen from q, broadcast; 0 where the numerator is 0"""
    A, B, C = a - q, b - q, c - q
    x0 = B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1]
    x1 = B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2]
    x2 = B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]
    num = (A[..., 0] * x0 + A[..., 1] * x1) + A[..., 2] * x2
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
    with np.errstate(invalid="ignore"):
        out = (2.0 * np.arctan2(num, den)) / FOUR_PI
    return np.where(num == 0.0, 0.0, out)


def solid_angles(P, V, F):
    """(n, T): Omega_f / 4 pi of every face seen from every row of P"""
    q = np.asarray(P, dtype=np.float32).astype(np.float64)[:, None, :]
    v = np.asarray(V, dtype=np.float32).astype(np.float64)
    F = np.asarray(F)
    with np.errstate(invalid="ignore", over="ignore"):
        return _face_terms(q, v[F[:, 0]][None], v[F[:, 1]][None], v[F[:, 2]][None])


def exact(P, V, F, chunk=2048):
    """(w (n,), sum of |terms| (n,)): the terms added in ascending face id; NaN for a non-finite query"""
    P = np.asarray(P, dtype=np.float32)
    w, s = np.empty(P.shape[0]), np.empty(P.shape[0])
    for i in range(0, P.shape[0], chunk):
        t = solid_angles(P[i:i + chunk], V, F)
        w[i:i + chunk] = np.cumsum(t, axis=1)[:, -1]                  # cumsum adds in order; np.sum would add pairwise
        s[i:i + chunk] = np.abs(t).sum(1)
    bad = ~np.isfinite(P.astype(np.float64)).all(1)
    w[bad] = np.nan
    return w, s


def build_tree(V, F):
    """a hierarchy in the device's format over (V, F): median splits of the centroids along the longest axis of their box, internal
    nodes numbered in pre-order, the leaves left to right"""
    V = np.asarray(V, dtype=np.float32)
    F = np.asarray(F)
    T = F.shape[0]
    v = V.astype(np.float64)
    cen = v[F].mean(1)
    left, right = np.zeros(max(T - 1, 0), np.int32), np.zeros(max(T - 1, 0), np.int32)
    tri = np.zeros(T, np.int32)
    counter = [0, 0]

    def rec(ids):
        if ids.size == 1:
            k = counter[1]
            counter[1] += 1
            tri[k] = ids[0]
            return T - 1 + k
        node = counter[0]
        counter[0] += 1
        c = cen[ids]
        ax = int(np.argmax(c.max(0) - c.min(0)))
        o = ids[np.argsort(c[:, ax], kind="stable")]
        h = o.size // 2
        left[node] = rec(o[:h])
        right[node] = rec(o[h:])
        return node

    rec(np.arange(T))
    N = 2 * T - 1
    parent = np.full(N, -1)
    parent[left], parent[right] = np.arange(T - 1), np.arange(T - 1)
    esc = np.full(N, -1, np.int32)
    for i in range(1, N):
        x = i
        while x != 0:
            p = parent[x]
            if left[p] == x:
                esc[i] = right[p]
                break
            x = p
    box = np.zeros((N, 6), np.float32)
    corners = V[F[tri]]
    box[T - 1:, :3], box[T - 1:, 3:] = corners.min(1), corners.max(1)
    lo, hi = ranges(dict(left=left, right=right), T)
    for i in range(T - 1):
        box[i, :3], box[i, 3:] = box[T - 1 + lo[i]:T + hi[i], :3].min(0), box[T - 1 + lo[i]:T + hi[i], 3:].max(0)
    return dict(left=left, right=right, esc=esc, tri=tri, box=box, V=V, F=F)


def ranges(arrays, T):
    """(lo, hi) per node: the leaves lo .. hi under it (a node's leaves are contiguous, the left child's first)"""
    N = 2 * T - 1
    lo, hi = np.zeros(N, np.int64), np.zeros(N, np.int64)
    lo[T - 1:] = hi[T - 1:] = np.arange(T)
    left, right = arrays["left"], arrays["right"]
    order, stack = [], [0] if T > 1 else []
    while stack:
        x = stack.pop()
        order.append(x)
        for c in (left[x], right[x]):
            if c < T - 1:
                stack.append(int(c))
    for x in reversed(order):
        assert lo[right[x]] == hi[left[x]] + 1
        lo[x], hi[x] = lo[left[x]], hi[right[x]]
    return lo, hi


def moments(arrays, V=None, F=None):
    """(2 T - 1, 36): every node's moments from their definitions, each a sum over the node's own faces about its own p"""
    V = arrays["V"] if V is None else V
    F = arrays["F"] if F is None else F
    v = np.asarray(V, dtype=np.float32).astype(np.float64)
    F = np.asarray(F)
    T = F.shape[0]
    N = 2 * T - 1
    box = arrays["box"].astype(np.float64).reshape(N, 6)
    o = (v.min(0) + v.max(0)) / 2                                     # the definitions do not depend on it; it keeps the sums small
    y = v[F[arrays["tri"]]] - o                                       # (T, 3 corners, 3), leaf order
    a = 0.5 * np.cross(y[:, 1] - y[:, 0], y[:, 2] - y[:, 0])
    ar = np.sqrt(_dot(a, a))
    cen = y.sum(1) / 3.0
    lo, hi = ranges(arrays, T)
    size = hi - lo + 1
    start = np.cumsum(size) - size
    node = np.repeat(np.arange(N), size)
    leaf = lo[node] + (np.arange(size.sum()) - start[node])

    def per_node(x):
        return np.add.reduceat(x, start, axis=0)

    m = np.zeros((N, STRIDE))
    Nv, Ar = per_node(a[leaf]), per_node(ar[leaf])
    with np.errstate(invalid="ignore", divide="ignore"):
        p = per_node((ar[:, None] * cen)[leaf]) / Ar[:, None]
    none = Ar == 0
    p[none] = (box[none, :3] + box[none, 3:]) / 2 - o
    yc = y[leaf] - p[node][:, None, :]                                # corners relative to the node's p
    cc = cen[leaf] - p[node]
    al = a[leaf]
    m[:, P_:P_ + 3] = p + o
    e = np.maximum(np.abs(m[:, :3] - box[:, :3]), np.abs(box[:, 3:] - m[:, :3]))
    m[:, R_] = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    m[:, N_:N_ + 3], m[:, AR_] = Nv, Ar
    m[:, C_:C_ + 9] = per_node((al[:, :, None] * cc[:, None, :]).reshape(-1, 9))
    for k, (i, j) in enumerate(SYM):
        s = ((yc[:, :, i] * yc[:, :, j]).sum(1) + 9.0 * cc[:, i] * cc[:, j]) / 12.0
        m[:, [T_ + k, T_ + 6 + k, T_ + 12 + k]] = per_node(al * s[:, None])
    return m


def far(m, rho, d2, d):
    """4 pi w_far of the nodes with moment rows m seen along rho = p - q (rows), d2 = |rho|^2, d = sqrt(d2)"""
    i2 = 1.0 / d2
    i3 = i2 / d
    i5 = i3 * i2
    i7 = i5 * i2
    t1 = _dot(rho, m[:, N_:N_ + 3]) * i3
    C = m[:, C_:C_ + 9].reshape(-1, 3, 3)
    tr = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    quad = sum(rho[:, i] * _dot(C[:, i], rho) for i in range(3))
    t2 = tr * i3 - 3.0 * (quad * i5)
    lin, cub = 0.0, 0.0
    r0, r1, r2 = rho[:, 0], rho[:, 1], rho[:, 2]
    for i in range(3):
        t00, t01, t02, t11, t12, t22 = (m[:, T_ + 6 * i + k] for k in range(6))
        row = [(t00 * r0 + t01 * r1) + t02 * r2, (t01 * r0 + t11 * r1) + t12 * r2, (t02 * r0 + t12 * r1) + t22 * r2][i]
        lin = lin + (2.0 * row + rho[:, i] * ((t00 + t11) + t22))
        qd = ((t00 * (r0 * r0) + t11 * (r1 * r1)) + t22 * (r2 * r2)) + 2.0 * ((t01 * (r0 * r1) + t02 * (r0 * r2)) + t12 * (r1 * r2))
        cub = cub + rho[:, i] * qd
    t3 = 0.5 * (15.0 * (cub * i7) - 3.0 * (lin * i5))
    return (t1 + t2) + t3


def walk(P, arrays, mom, beta):
    """(w (n,), sum of |terms| (n,), nodes accepted (n,), leaves visited (n,)): the walk of every row of P over the hierarchy with the
    moments `mom`, all queries stepping together; a query's terms are added in its own visiting order"""
    P = np.asarray(P, dtype=np.float32)
    q = P.astype(np.float64)
    v = np.asarray(arrays["V"], dtype=np.float32).astype(np.float64)
    F, tri, left, esc = np.asarray(arrays["F"]), arrays["tri"], arrays["left"], arrays["esc"]
    T = F.shape[0]
    leaf0 = T - 1
    n = q.shape[0]
    w, s = np.zeros(n), np.zeros(n)
    accepted, leaves = np.zeros(n, np.int64), np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    finite = np.isfinite(q).all(1)
    node[~finite] = -1
    while True:
        act = np.nonzero(node >= 0)[0]
        if act.size == 0:
            break
        nd = node[act]
        m = mom[nd]
        rho = m[:, P_:P_ + 3] - q[act]
        d2 = (rho[:, 0] * rho[:, 0] + rho[:, 1] * rho[:, 1]) + rho[:, 2] * rho[:, 2]
        d = np.sqrt(d2)
        acc = d > beta * m[:, R_]
        isleaf = ~acc & (nd >= leaf0)
        term = np.zeros(act.size)
        if acc.any():
            term[acc] = far(m[acc], rho[acc], d2[acc], d[acc]) / FOUR_PI
        if isleaf.any():
            f = F[tri[nd[isleaf] - leaf0]]
            term[isleaf] = _face_terms(q[act[isleaf]], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
        w[act] += term
        s[act] += np.abs(term)
        accepted[act] += acc
        leaves[act] += isleaf
        done = acc | isleaf
        nxt = np.where(done, esc[nd], left[np.minimum(nd, max(T - 2, 0))] if T > 1 else -1)
        node[act] = nxt
    w[~finite] = np.nan
    return w, s, accepted, leaves
