"""The rule of csrc/topology.hip restated in numpy: a plain union-find, a dictionary of edges and a walk of the
boundary loops -- no scipy, nothing of the device's sorts, scans or hooking. Every array is integer-valued with one right answer, and the
measures follow the device's order of additions, so the device must return exactly what is computed here. Also the small meshes the
tests share.

Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; the half-edges of one unordered pair form an edge, owned by the lowest h;
edges are numbered by ascending owner. Vertex components: joined by an edge, numbered by ascending lowest vertex. Facet components:
faces sharing an edge, numbered by ascending lowest face. A loop follows the boundary half-edges from its lowest vertex; loops by
ascending lowest vertex. Measures: per-face fp64 terms, per component summed over ascending face id -- at most 64 faces in order; more
by 64 lanes, lane l taking faces l, l + 64, ... in order, the lanes added by the xor butterfly 32, 16, ... 1 (seg_sum of groupby.h)."""
import numpy as np

BOUNDARY, NONMANIFOLD, MISORIENTED = 1, 2, 4
BAD_BOUNDARY = "boundary is not a set of oriented cycles"


class UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)

    def labels(self):
        """the components numbered by ascending lowest member (a root is the lowest member of its set: union hangs the larger below)"""
        n = len(self.p)
        roots = [self.find(i) for i in range(n)]
        number = {r: k for k, r in enumerate(sorted(set(roots)))}
        return np.array([number[r] for r in roots], dtype=np.int64), len(number)


class Topology:
    """what largesteps.topology.MeshTopology(F, V) holds; raises ValueError as its constructor does"""

    def __init__(self, F, V):
        F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
        m, V = F.shape[0], int(V)
        if m and (F.min() < 0 or F.max() >= V):
            raise ValueError("index out of range")
        if m and ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])).any():
            raise ValueError("a face names a vertex twice")
        self.F, self.V, self.m = F, V, m
        tri = F.reshape(-1)
        head = F[:, [1, 2, 0]].reshape(-1)
        groups = {}                                          # (lower end, higher end) -> its half-edges, ascending; in order of their owners
        for h in range(3 * m):
            a, b = int(tri[h]), int(head[h])
            groups.setdefault((min(a, b), max(a, b)), []).append(h)
        self.E = len(groups)
        self.edges = np.array(list(groups), dtype=np.int64).reshape(-1, 2)
        self.edge_faces = -np.ones((self.E, 2), dtype=np.int64)
        self.eflag = np.zeros(self.E, dtype=np.int64)
        vu, fu = UnionFind(V), UnionFind(m)
        bnext, b_out, b_in = {}, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
        for e, ((a, b), g) in enumerate(groups.items()):
            vu.union(a, b)
            for h0, h1 in zip(g[:-1], g[1:]):
                fu.union(h0 // 3, h1 // 3)
            self.edge_faces[e, :min(len(g), 2)] = [h // 3 for h in g[:2]]
            if len(g) == 1:
                self.eflag[e] = BOUNDARY
                s, t = int(tri[g[0]]), int(head[g[0]])
                bnext[s] = t
                b_out[s] += 1
                b_in[t] += 1
            elif len(g) > 2:
                self.eflag[e] = NONMANIFOLD
            elif tri[g[0]] == tri[g[1]]:
                self.eflag[e] = MISORIENTED
        self.vertex_components, self.num_vertex_components = vu.labels()
        self.facet_components, self.num_facet_components = fu.labels()
        self.num_boundary_edges = int((self.eflag == BOUNDARY).sum())
        self.num_nonmanifold_edges = int((self.eflag == NONMANIFOLD).sum())
        self.num_misoriented_edges = int((self.eflag == MISORIENTED).sum())
        self.is_edge_manifold = self.num_nonmanifold_edges == 0
        self.is_oriented = self.is_edge_manifold and self.num_misoriented_edges == 0
        self.is_closed = self.num_boundary_edges == 0
        on = (b_out > 0) | (b_in > 0)
        self.loops_defined = bool(((b_out[on] == 1) & (b_in[on] == 1)).all())
        self._bnext = bnext

    def counts(self):
        K, fc = self.num_facet_components, self.facet_components
        c = np.zeros((K, 6), dtype=np.int64)
        for k in range(K):
            faces = self.F[fc == k]
            c[k, 0] = faces.shape[0]
            c[k, 1] = np.unique(faces).size
        for e in range(self.E):
            k = fc[self.edge_faces[e, 0]]
            c[k, 2] += 1
            c[k, 3] += self.eflag[e] == BOUNDARY
            c[k, 4] += self.eflag[e] == NONMANIFOLD
            c[k, 5] += self.eflag[e] == MISORIENTED
        return c

    def euler_characteristic(self):
        c = self.counts()
        return c[:, 1] - c[:, 2] + c[:, 0]

    def boundary_loops(self):
        """(loops (B,), ptr (L + 1,))"""
        if not self.loops_defined:
            raise ValueError(BAD_BOUNDARY)
        seen, loops, ptr = set(), [], [0]
        for v in sorted(self._bnext):                        # an unseen vertex in ascending order is the lowest of its loop
            if v in seen:
                continue
            u = v
            while u not in seen:
                seen.add(u)
                loops.append(u)
                u = self._bnext[u]
            assert u == v
            ptr.append(len(loops))
        return np.array(loops, dtype=np.int64), np.array(ptr, dtype=np.int64)

    def loop_list(self):
        loops, ptr = self.boundary_loops()
        return [loops[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]

    def keep(self, mask):
        """(F2, I, J)"""
        mask = np.asarray(mask, dtype=bool)
        assert mask.shape == (self.num_facet_components,)
        kept = self.F[mask[self.facet_components]] if self.m else self.F
        J = np.unique(kept)
        I = -np.ones(self.V, dtype=np.int64)
        I[J] = np.arange(J.size)
        return I[kept].reshape(-1, 3), I, J


# ---- measures ---------------------------------------------------------------------------------------------------------------------------
def face_terms(V, F):
    """(m, 2) fp64: the area and volume terms of every face, every sum and product in the device's order"""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    x = np.asarray(V, dtype=np.float32).astype(np.float64)
    a, b, c = x[F[:, 0]], x[F[:, 1]], x[F[:, 2]]
    u, v = b - a, c - a
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    kx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    ky = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    kz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    vol = ((a[:, 0] * kx + a[:, 1] * ky) + a[:, 2] * kz) / 6.0
    return np.stack([area, vol], axis=1)


def seg_sum(terms):
    """the sum of the rows of terms (n, C) fp64, from 0, in the order of seg_sum (groupby.h)"""
    def run(rows):
        acc = np.zeros(terms.shape[1], dtype=np.float64)
        for t in rows:
            acc = acc + t
        return acc
    if terms.shape[0] <= 64:
        return run(terms)
    lanes = np.stack([run(terms[l::64]) for l in range(64)])
    m = 32
    while m >= 1:
        lanes = lanes + lanes[np.arange(64) ^ m]
        m >>= 1
    return lanes[0]


def measures(T, V):
    """(K, 2) fp64: area and signed volume of every facet component of the Topology T at the positions V"""
    terms = face_terms(V, T.F)
    out = np.zeros((T.num_facet_components, 2), dtype=np.float64)
    for k in range(T.num_facet_components):
        out[k] = seg_sum(terms[T.facet_components == k])
    return out


def largest(T, V, by):
    """the mask of keep_largest_component: ties go to the lower component id"""
    key = T.counts()[:, 0] if by == "faces" else measures(T, V)[:, 0] if by == "area" else np.abs(measures(T, V)[:, 1])
    mask = np.zeros(T.num_facet_components, dtype=bool)
    mask[int(np.argmax(key))] = True
    return mask


# ---- the meshes -------------------------------------------------------------------------------------------------------------------------
def positions(V, seed=0):
    return np.random.default_rng(seed).standard_normal((V, 3)).astype(np.float32)


def torus(n=6, m=5):
    """(F, V) of an n x m grid of quads closed both ways, consistently wound"""
    idx = lambda i, j: (i % n) * m + (j % m)
    F = []
    for i in range(n):
        for j in range(m):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            F += [[a, b, c], [a, c, d]]
    return np.array(F, dtype=np.int64), n * m


def moebius(n=8):
    """(F, V) of a strip of n quads whose ends are glued with a half twist: rows (2 i, 2 i + 1), the last quad joins row n - 1 to
    row 0 upside down. One facet component, one side: some edge is misoriented whichever way the faces are wound."""
    F = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        if i + 1 < n:
            c, d = 2 * (i + 1), 2 * (i + 1) + 1
        else:
            c, d = 1, 0
        F += [[a, c, d], [a, d, b]]
    return np.array(F, dtype=np.int64), 2 * n


def strip(n):
    """(F, V): n triangles in a row over n + 2 vertices, (i, i + 1, i + 2) wound alternately so that the strip is oriented"""
    F = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)], dtype=np.int64)
    return F, n + 2


def renumbered(F, V, perm, face_perm=None):
    """the mesh with vertex v called perm[v], its faces in the order face_perm"""
    F = np.asarray(perm, dtype=np.int64)[F]
    return (F if face_perm is None else F[face_perm]), V


def without_cells(n, cells):
    """plane(n)'s faces without the two triangles of every cell (x, y) in cells"""
    from largesteps import synthetic
    F = synthetic.plane(n)[1].astype(np.int64)
    drop = np.zeros(F.shape[0], dtype=bool)
    for x, y in cells:
        c = y * (n - 1) + x
        drop[2 * c:2 * c + 2] = True
    return F[~drop], n * n


def hollow_ball(n=3):
    """(V fp32, F): icosphere(n) and an inward-flipped copy at radius 1/2"""
    from largesteps import synthetic
    v, f = synthetic.icosphere(n)
    f = f.astype(np.int64)
    return np.concatenate([v, 0.5 * v]).astype(np.float32), np.concatenate([f, f[:, ::-1] + v.shape[0]])


def tetrahedra(k, V=None, seed=0):
    """(F, V): k disjoint tetrahedra; with V given, on random distinct ids below V (the other vertices are in no face)"""
    base = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)
    F = np.concatenate([base + 4 * i for i in range(k)])
    if V is None:
        return F, 4 * k
    ids = np.random.default_rng(seed).permutation(V)[:4 * k]
    return ids[F], V


def small_meshes():
    """name -> (F int64, V): every way the rule can go at the smallest size"""
    from largesteps import synthetic
    tet = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)
    cone = lambda tip, rim: [[tip, rim[i], rim[(i + 1) % len(rim)]] for i in range(len(rim))]
    shells = synthetic.shells(2)
    return {
        "tetrahedron": (tet, 4),
        "two_tetrahedra": (np.concatenate([tet, tet + 4]), 8),
        "cones_tip_to_tip": (np.array(cone(0, [1, 2, 3, 4]) + cone(0, [8, 7, 6, 5]), dtype=np.int64), 9),
        "three_faces_on_an_edge": (np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64), 5),
        "same_direction": (np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int64), 4),
        "moebius8": moebius(8),
        "plane4": (synthetic.plane(4)[1].astype(np.int64), 16),
        "plane6_hole": without_cells(6, [(2, 2)]),                                   # two faces removed in the middle
        "shells2": (shells[1].astype(np.int64), shells[0].shape[0]),
        "icosphere2": (synthetic.icosphere(2)[1].astype(np.int64), 42),
        "torus": torus(),
        "unreferenced": (np.array([[2, 3, 5], [2, 5, 6], [9, 10, 8]], dtype=np.int64), 13),      # 0, 1 before; 4, 7 between; 11, 12 after
        "bowtie": (np.array([[0, 1, 2], [0, 3, 4]], dtype=np.int64), 5),          # a boundary vertex with two half-edges leaving
        "empty": (np.zeros((0, 3), dtype=np.int64), 5),
    }
