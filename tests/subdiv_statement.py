"""The rule of csrc/subdiv.hip restated in numpy, and the same map a second time as a dense matrix built from a
Python dict of edges. The statement follows the device's order of additions, so the device must return its bits; the dense matrix
shares nothing with the statement's walk and checks the statement itself. Also the small meshes the tests of both share.

Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; the half-edges of one unordered pair form an edge, owned by the lowest
id; edges are numbered by ascending owner. The walk of a vertex: its corners by ascending corner id, at each corner the outgoing
half-edge 3 f + i and then the incoming one 3 f + (i + 2) % 3, an edge counted only at its owner. More than 64 corners: lane l of 64 takes
corners l, l + 64, ... in order, and the lanes are added by the xor butterfly 32, 16, ... 1."""
import numpy as np

MIDPOINT, LOOP = "midpoint", "loop"


def beta(n):
    return 3.0 / 16.0 if n == 3 else 3.0 / (8.0 * float(n))


class Topology:
    """one level over faces F (m, 3) and V vertices; raises ValueError as the constructor of largesteps.subdivide.Subdivision does"""

    def __init__(self, F, V):
        F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
        m = F.shape[0]
        if m and (F.min() < 0 or F.max() >= V):
            raise ValueError("index out of range")
        if m and ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])).any():
            raise ValueError("a face names a vertex twice")
        self.F, self.V, self.m = F, int(V), m
        n = 3 * m
        tri = F.reshape(-1)
        head = F[:, [1, 2, 0]].reshape(-1)                    # where half-edge h ends
        groups = {}
        for h in range(n):
            a, b = int(tri[h]), int(head[h])
            groups.setdefault((min(a, b), max(a, b)), []).append(h)
        if any(len(g) > 2 for g in groups.values()):
            raise ValueError("non-manifold edge")
        owner = np.zeros(n, dtype=bool)
        mate = -np.ones(n, dtype=np.int64)
        for g in groups.values():
            owner[g[0]] = True
            if len(g) == 2:
                mate[g[0]], mate[g[1]] = g[1], g[0]
        first = np.cumsum(owner) - owner                      # the exclusive scan of the owner flags
        self.owner, self.mate = owner, mate
        self.eid = np.where(owner, first, first[np.where(owner, 0, mate)]) if n else np.zeros(0, dtype=np.int64)
        self.boundary = mate < 0
        self.E = int(owner.sum())
        own = np.flatnonzero(owner)
        self.edges = np.stack([np.minimum(tri[own], head[own]), np.maximum(tri[own], head[own])], axis=1) if n else np.zeros((0, 2), np.int64)
        third = F[:, [2, 0, 1]].reshape(-1)                   # the corner opposite half-edge h
        self.opp = np.stack([third[own], np.where(mate[own] >= 0, third[np.maximum(mate[own], 0)], -1)], axis=1) if n else np.zeros((0, 2), np.int64)
        order = np.argsort(tri, kind="stable")
        vptr = np.concatenate([[0], np.cumsum(np.bincount(tri, minlength=self.V))]) if n else np.zeros(self.V + 1, dtype=np.int64)
        self.corners = [order[vptr[v]:vptr[v + 1]] for v in range(self.V)]
        self.valence = np.zeros(self.V, dtype=np.int64)
        self.bflag = np.zeros(self.V, dtype=bool)
        self.bnbr = -np.ones((self.V, 2), dtype=np.int64)
        for v in range(self.V):
            far = [u for _, u in self.owned(v)]
            bfar = [u for h, u in self.owned(v) if self.boundary[h]]
            if len(bfar) not in (0, 2):
                raise ValueError("non-manifold vertex")
            self.valence[v] = len(far)
            if bfar:
                self.bflag[v], self.bnbr[v] = True, bfar
        mid = self.V + self.eid.reshape(-1, 3) if n else np.zeros((0, 3), dtype=np.int64)
        fine = np.empty((m, 4, 3), dtype=np.int64)
        for e in range(3):
            fine[:, e] = np.stack([F[:, e], mid[:, e], mid[:, (e + 2) % 3]], axis=1)
        fine[:, 3] = mid
        self.faces = fine.reshape(-1, 3)

    def corner_halfedges(self, c):
        """(outgoing half-edge, its far end), (incoming half-edge, its far end), the opposite half-edge of corner c"""
        f, i = divmod(int(c), 3)
        h1, h2 = 3 * f + (i + 1) % 3, 3 * f + (i + 2) % 3
        return (int(c), int(self.F[f, (i + 1) % 3])), (h2, int(self.F[f, (i + 2) % 3])), h1

    def owned(self, v):
        """the walk of v: (owner half-edge, far end) of every edge at v"""
        out = []
        for c in self.corners[v]:
            o, i, _ = self.corner_halfedges(c)
            out += [x for x in (o, i) if self.owner[x[0]]]
        return out


def walk_sum(per_corner, C):
    """the sum of the terms of a walk, from 0, in the device's order: per_corner[j] is the list of the fp64 (C,) terms of corner j"""
    def run(corners):
        acc = np.zeros(C, dtype=np.float64)
        for terms in corners:
            for t in terms:
                acc = acc + t
        return acc
    if len(per_corner) <= 64:
        return run(per_corner)
    lanes = np.stack([run(per_corner[l::64]) for l in range(64)])
    m = 32
    while m >= 1:
        lanes = lanes + lanes[np.arange(64) ^ m]
        m >>= 1
    return lanes[0]


def apply(T, X, scheme):
    """S X: X (V, C) fp32 -> (V + E, C) fp32"""
    X = np.asarray(X, dtype=np.float32)
    x = X.astype(np.float64)
    C = X.shape[1]
    out = np.empty((T.V + T.E, C), dtype=np.float32)
    for v in range(T.V):
        n = int(T.valence[v])
        if scheme == MIDPOINT or n == 0:
            out[v] = X[v]
        elif T.bflag[v]:
            p, q = T.bnbr[v]
            out[v] = (0.75 * x[v] + 0.125 * (x[p] + x[q])).astype(np.float32)
        else:
            per_corner = []
            for c in T.corners[v]:
                o, i, _ = T.corner_halfedges(c)
                per_corner.append([x[u] for h, u in (o, i) if T.owner[h]])
            b = beta(n)
            w = 1.0 - float(n) * b
            out[v] = (w * x[v] + b * walk_sum(per_corner, C)).astype(np.float32)
    for e in range(T.E):
        a, b = T.edges[e]
        c, d = T.opp[e]
        if scheme == MIDPOINT or d < 0:
            out[T.V + e] = ((x[a] + x[b]) * 0.5).astype(np.float32)
        else:
            out[T.V + e] = (0.375 * (x[a] + x[b]) + 0.125 * (x[c] + x[d])).astype(np.float32)
    return out


def apply_transposed(T, g, scheme):
    """S^T g: g (V + E, C) fp32 -> (V, C) fp32, as the gather of the backward"""
    g32 = np.asarray(g, dtype=np.float32)
    g = g32.astype(np.float64)
    C = g.shape[1]
    loop = scheme == LOOP
    out = np.empty((T.V, C), dtype=np.float32)
    for v in range(T.V):
        per_corner = []
        for c in T.corners[v]:
            o, i, hf = T.corner_halfedges(c)
            terms = []
            for h, u in (o, i):
                if not T.owner[h]:
                    continue
                bnd = bool(T.boundary[h])
                if loop:
                    if not T.bflag[u]:
                        terms.append(beta(int(T.valence[u])) * g[u])
                    elif bnd:
                        terms.append(0.125 * g[u])
                terms.append((0.375 if loop and not bnd else 0.5) * g[T.V + T.eid[h]])
            if loop and not T.boundary[hf]:
                terms.append(0.125 * g[T.V + T.eid[hf]])
            per_corner.append(terms)
        n = int(T.valence[v])
        w = 1.0 if not loop or n == 0 else 0.75 if T.bflag[v] else 1.0 - float(n) * beta(n)
        out[v] = (w * g[v] + walk_sum(per_corner, C)).astype(np.float32)
    return out


def levels_of(F, V, levels):
    """the topologies of `levels` applications"""
    out = []
    for _ in range(levels):
        T = Topology(F, V)
        out.append(T)
        F, V = T.faces, T.V + T.E
    return out


def subdivide(F, V, X, scheme, levels=1):
    """(X_fine, F_fine) of `levels` applications"""
    F = np.asarray(F, dtype=np.int64)
    for T in levels_of(F, V, levels):
        X, F = apply(T, X, scheme), T.faces
    return X, F


def dense_matrix(F, V, scheme):
    """S (V + E, V) fp64 from a dict of edges: no corner ranking, no half-edge flags. Edges are numbered in the order their first
    half-edge appears, which is the order of their owners."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    opposite = {}
    for face in F:
        for e in range(3):
            a, b, c = int(face[e]), int(face[(e + 1) % 3]), int(face[(e + 2) % 3])
            opposite.setdefault((min(a, b), max(a, b)), []).append(c)
    E = len(opposite)
    S = np.zeros((V + E, V), dtype=np.float64)
    nbrs = {v: [] for v in range(V)}
    bnbrs = {v: [] for v in range(V)}
    for k, ((a, b), cs) in enumerate(opposite.items()):
        nbrs[a].append(b)
        nbrs[b].append(a)
        if len(cs) == 1:
            bnbrs[a].append(b)
            bnbrs[b].append(a)
        if scheme == MIDPOINT or len(cs) == 1:
            S[V + k, a] += 0.5
            S[V + k, b] += 0.5
        else:
            S[V + k, a] += 0.375
            S[V + k, b] += 0.375
            S[V + k, cs[0]] += 0.125
            S[V + k, cs[1]] += 0.125
    for v in range(V):
        n = len(nbrs[v])
        if scheme == MIDPOINT or n == 0:
            S[v, v] = 1.0
        elif bnbrs[v]:
            S[v, v] = 0.75
            for u in bnbrs[v]:
                S[v, u] += 0.125
        else:
            b = beta(n)
            S[v, v] = 1.0 - n * b
            for u in nbrs[v]:
                S[v, u] += b
    return S


# ---- the meshes ------------------------------------------------------------------------------------------------------------------------
def fan(k):
    """k faces around the interior vertex 0, closed: its valence k, a rim of k boundary vertices"""
    F = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], dtype=np.int64)
    return F, k + 1


def small_meshes():
    """name -> (F int64, V): every branch of the rule at the smallest size"""
    from largesteps import synthetic
    ico = synthetic.icosphere(1)[1]
    plane = synthetic.plane(4)[1]
    return {
        "tetrahedron": (np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64), 4),                       # valence 3
        "octahedron": (np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64), 6),
        "icosphere1": (ico.astype(np.int64), 12),                                                                         # valence 5
        "icosphere2": (synthetic.icosphere(2)[1].astype(np.int64), 42),                                                   # valences 5 and 6
        "triangle": (np.array([[0, 1, 2]], dtype=np.int64), 3),                                                           # all boundary
        "two_triangles": (np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64), 4),                    # boundary vertices with an interior edge
        "plane4": (plane.astype(np.int64), 16),
        "flipped_quad": (np.array([[0, 1, 2], [0, 3, 2]], dtype=np.int64), 4),                                            # inconsistent winding
        "unreferenced": (np.array([[1, 2, 4], [1, 4, 5]], dtype=np.int64), 7),                                            # 0, 3, 6 in no face
        "fan5": (fan(5)[0], 6),
    }


def values(V, C, seed):
    return np.random.default_rng(seed).standard_normal((V, C)).astype(np.float32)
