"""
Statement of the isosurface extractor of largesteps.levelset (csrc/isosurf.hip) in numpy: marching tetrahedra on
the Kuhn split of a regular grid, with the fp32 operations of the device code in its order (the build has -ffp-contract=off). No device.

1. Grid. S is (nx, ny, nz) fp32; node (i, j, k) lies at origin + spacing * (i, j, k) and has id (i ny + j) nz + k. A cube is the 8 nodes
   c + {0, 1}^3 for c < (nx - 1, ny - 1, nz - 1), its id (i (ny - 1) + j) (nz - 1) + k; its corner (di, dj, dk) has number 4 di + 2 dj + dk.
   A grid with a side of 1 has no cubes and, by definition, no vertices either.
2. Tets. Every cube splits into the 6 Kuhn tets v0 = c, v1 = c + e_a, v2 = c + e_a + e_b, v3 = c + (1, 1, 1), one per permutation
   (a, b, .) of the axes in lexicographic order (PERMS). The tet is positively oriented iff the permutation is even. Its 6 edges are
   (v0 v1, v0 v2, v0 v3, v1 v2, v1 v3, v2 v3) = edges 0..5; each runs from the lower corner to the higher along one of the 7 directions
   100, 010, 001, 110, 011, 101, 111 = slots 0..6, and the node it starts at OWNS it.
3. Low, high, live. iso is rounded to fp32. A node is low iff S < iso, else high (a NaN is high). An edge is live iff both ends are
   finite and exactly one is low. A cube with a non-finite corner emits nothing.
4. Vertices. One per live edge, ordered by (owning node id, slot): index = offs[node] + popcount(mask[node] & ((1 << slot) - 1)), mask the
   7-bit live mask of the node and offs the exclusive scan of its popcounts. With a the owning node, b = a + d, all fp32:
   t = (iso - S[a]) / (S[b] - S[a]); t = t if t > 0 else 0; t = t if t < 1 else 1; per axis x = origin + spacing * ((float) i_a + t d).
   E = 8 node + slot.
5. Faces. Ordered by (cube id, tet, triangle). With the 4-bit case of a tet (bit i set iff v_i is low): one low or one high corner gives
   one triangle, two and two give a quad cut into two triangles. For a positive tet, LONE[i] lists the other three corners in the
   order in which (edge to o0, edge to o1, edge to o2) has its normal pointing away from v_i: that is the triangle of a lone LOW v_i, and
   a lone HIGH v_i takes (o0, o2, o1). For low {a, b}, PAIR gives (c, d) with (a, b, c, d) an even permutation: the quad is
   (ac, ad, bd, bc), cut along ac - bd into (ac, ad, bd) and (ac, bd, bc). A negative tet swaps the last two corners of every triangle.
   So every face's normal points from the low side to the high side.
6. Gradient of V in S, gS = sum_v <gV[v], dV[v] / dS>, in fp64 from the fp32 inputs: for a live edge with D = S[b] - S[a], t = (iso - S[a]) / D
   (in fp64; the term is zero unless 0 <= t <= 1), e = spacing * d, ge = (gV_x e_x + gV_y e_y) + gV_z e_z:
   term_a = (-(1 - t) / D) * ge, term_b = (-t / D) * ge. A node adds the term_a of its 7 owned slots in order, then the term_b of the 7
   edges owned by node - d in slot order, in fp64, and the sum is rounded to fp32 once. A vertex past n adds nothing.
"""
import itertools

import numpy as np

F32 = np.float32
SLOTS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]], dtype=np.int64)
PERMS = list(itertools.permutations(range(3)))                     # lexicographic
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
LONE = {0: (1, 2, 3), 1: (0, 3, 2), 2: (0, 1, 3), 3: (0, 2, 1)}
PAIR = {(0, 1): (2, 3), (0, 2): (3, 1), (0, 3): (1, 2), (1, 2): (0, 3), (1, 3): (2, 0), (2, 3): (0, 1)}


def _slot_of(d):
    return int(np.flatnonzero((SLOTS == np.asarray(d)).all(1))[0])


def _edge(x, y):
    return EDGES.index((min(x, y), max(x, y)))


def _tables():
    corners = np.zeros((6, 4), np.int64)           # tet -> the cube corner numbers of v0..v3
    owner = np.zeros((6, 6), np.int64)             # tet, edge -> the cube corner that owns it
    slot = np.zeros((6, 6), np.int64)              # tet, edge -> its slot
    sign = np.zeros(6, np.int64)
    for t, (a, b, c) in enumerate(PERMS):
        v = np.zeros((4, 3), np.int64)
        v[1, a] = 1
        v[2, a] = v[2, b] = 1
        v[3] = 1
        corners[t] = 4 * v[:, 0] + 2 * v[:, 1] + v[:, 2]
        sign[t] = round(np.linalg.det(np.stack([np.eye(3)[a], np.eye(3)[b], np.eye(3)[c]])))
        for e, (x, y) in enumerate(EDGES):
            owner[t, e] = corners[t, x]
            slot[t, e] = _slot_of(v[y] - v[x])
    ntri = np.zeros(16, np.int64)
    tris = np.zeros((16, 2, 3), np.int64)          # case -> its triangles as tet edges, for a positive tet
    for case in range(1, 15):
        low = [i for i in range(4) if case >> i & 1]
        high = [i for i in range(4) if not case >> i & 1]
        if len(low) == 1 or len(high) == 1:
            i = low[0] if len(low) == 1 else high[0]
            o = LONE[i] if len(low) == 1 else (LONE[i][0], LONE[i][2], LONE[i][1])
            ntri[case] = 1
            tris[case, 0] = [_edge(i, o[0]), _edge(i, o[1]), _edge(i, o[2])]
        else:
            a, b = low
            c, d = PAIR[(a, b)]
            ntri[case] = 2
            tris[case, 0] = [_edge(a, c), _edge(a, d), _edge(b, d)]
            tris[case, 1] = [_edge(a, c), _edge(b, d), _edge(b, c)]
    return corners, owner, slot, sign, ntri, tris


TET_CORNERS, TET_EDGE_OWNER, TET_EDGE_SLOT, TET_SIGN, NTRI, TRIS = _tables()


def packed_tables():
    """the tables as the device source holds them: per case bits 3 j .. 3 j + 2 = tet edge of triangle corner j (j = 0..5) and bits 18..19
    the number of triangles; per tet 6 bits per edge (owner corner, slot << 3) and 3 bits per corner; the mask of negative tets"""
    case = [int(sum(int(TRIS[c].reshape(-1)[j]) << (3 * j) for j in range(6)) | int(NTRI[c]) << 18) for c in range(16)]
    edge = [int(sum((int(TET_EDGE_OWNER[t, e]) | int(TET_EDGE_SLOT[t, e]) << 3) << (6 * e) for e in range(6))) for t in range(6)]
    corner = [int(sum(int(TET_CORNERS[t, i]) << (3 * i) for i in range(4))) for t in range(6)]
    neg = int(sum(1 << t for t in range(6) if TET_SIGN[t] < 0))
    return case, edge, corner, neg


_POP = np.array([bin(i).count("1") for i in range(128)], dtype=np.int64)


def _spacing3(spacing):
    s = np.asarray(spacing, dtype=np.float64).reshape(-1)
    return np.array([s[0]] * 3 if s.size == 1 else s, dtype=F32)


def classify(S, iso):
    """(mask (N,) uint8, offs (N + 1,) int64): the live masks of the nodes and the exclusive scan of their popcounts"""
    S = np.asarray(S, dtype=F32)
    nx, ny, nz = S.shape
    iso = F32(iso)
    mask = np.zeros((nx, ny, nz), np.uint8)
    if min(nx, ny, nz) > 1:
        fin = np.isfinite(S)
        with np.errstate(invalid="ignore"):
            low = S < iso
        for s, (dx, dy, dz) in enumerate(SLOTS):
            A = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
            B = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
            live = fin[A] & fin[B] & (low[A] ^ low[B])
            mask[A] |= (live.astype(np.uint8) << s).astype(np.uint8)
    mask = mask.reshape(-1)
    offs = np.concatenate([[0], np.cumsum(_POP[mask])]).astype(np.int64)
    return mask, offs


def _rank(mask, offs, node, slot):
    return offs[node] + _POP[mask[node] & ((1 << slot) - 1)]


def _edge_ends(S, slot):
    """for every node the id of node + d (clipped where it leaves the grid: such an edge is never live)"""
    nx, ny, nz = S.shape
    dx, dy, dz = SLOTS[slot]
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return ((np.minimum(i + dx, nx - 1) * ny + np.minimum(j + dy, ny - 1)) * nz + np.minimum(k + dz, nz - 1)).reshape(-1)


def extract(S, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, with_tets=False):
    """(V (n, 3) fp32, E (n,) int64, F (m, 3) int64) of rules 1 to 5; with_tets adds T (m,) int64 = 6 cube + tet, the tet of every face"""
    S = np.ascontiguousarray(S, dtype=F32)
    nx, ny, nz = S.shape
    iso = F32(iso)
    o, sp = np.asarray(origin, dtype=F32), _spacing3(spacing)
    mask, offs = classify(S, iso)
    n = int(offs[-1])
    Sf = S.reshape(-1)
    V, E = np.zeros((n, 3), F32), np.zeros(n, np.int64)
    node = np.arange(nx * ny * nz)
    ijk = np.stack(np.unravel_index(node, (nx, ny, nz)), 1)
    for s in range(7):
        a = node[(mask >> s & 1) == 1]
        b = _edge_ends(S, s)[a]
        with np.errstate(all="ignore"):
            t = (iso - Sf[a]) / (Sf[b] - Sf[a])
        t = np.where(t > 0, t, F32(0))
        t = np.where(t < 1, t, F32(1)).astype(F32)
        idx = _rank(mask, offs, a, s)
        for ax in range(3):
            V[idx, ax] = o[ax] + sp[ax] * (ijk[a, ax].astype(F32) + t * F32(SLOTS[s, ax]))
        E[idx] = 8 * a + s
    # faces
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    if min(cx, cy, cz) < 1:
        return (V, E, np.zeros((0, 3), np.int64)) + ((np.zeros(0, np.int64),) if with_tets else ())
    fin = np.isfinite(S)
    with np.errstate(invalid="ignore"):
        low = S < iso
    ok = np.ones((cx, cy, cz), bool)
    low8 = np.zeros((cx, cy, cz), np.int64)
    for c in range(8):
        di, dj, dk = c >> 2 & 1, c >> 1 & 1, c & 1
        sl = (slice(di, di + cx), slice(dj, dj + cy), slice(dk, dk + cz))
        ok &= fin[sl]
        low8 |= low[sl].astype(np.int64) << c
    ok, low8 = ok.reshape(-1), low8.reshape(-1)
    ci, cj, ck = np.unravel_index(np.arange(cx * cy * cz), (cx, cy, cz))
    base = (ci * ny + cj) * nz + ck                                     # node id of the cube's corner 0
    case = np.zeros((6, cx * cy * cz), np.int64)
    for t in range(6):
        for i in range(4):
            case[t] |= (low8 >> TET_CORNERS[t, i] & 1) << i
    nt = np.where(ok[None], NTRI[case], 0)
    before = np.cumsum(nt, 0) - nt                                     # triangles of the cube's earlier tets
    coffs = np.concatenate([[0], np.cumsum(nt.sum(0))])
    m = int(coffs[-1])
    F, T = np.zeros((m, 3), np.int64), np.zeros(m, np.int64)
    for t in range(6):
        for j in range(2):
            sel = np.flatnonzero(nt[t] > j)
            row = coffs[sel] + before[t, sel] + j
            T[row] = 6 * sel + t
            for c in range(3):
                cc = c if TET_SIGN[t] > 0 or c == 0 else 3 - c
                e = TRIS[case[t, sel], j, cc]
                corner = TET_EDGE_OWNER[t, e]
                nd = base[sel] + ((corner >> 2 & 1) * ny + (corner >> 1 & 1)) * nz + (corner & 1)
                F[row, c] = offs[nd] + _POP[mask[nd] & ((1 << TET_EDGE_SLOT[t, e]) - 1)]
    return (V, E, F, T) if with_tets else (V, E, F)


def tet_nodes(shape, T):
    """(m, 4) node ids of the corners v0..v3 of the tets T = 6 cube + tet"""
    nx, ny, nz = shape
    ci, cj, ck = np.unravel_index(np.asarray(T) // 6, (nx - 1, ny - 1, nz - 1))
    corner = TET_CORNERS[np.asarray(T) % 6]
    return ((ci[:, None] + (corner >> 2 & 1)) * ny + cj[:, None] + (corner >> 1 & 1)) * nz + ck[:, None] + (corner & 1)


def level_set_grid(V, h, pad=2):
    """the grid of largesteps.levelset.remesh_level_set over the mesh vertices V: (origin (3,) fp64, dims (3,) int, P (N, 3) fp32 nodes)"""
    v = np.asarray(V, dtype=F32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    origin = lo - pad * h
    dims = np.ceil((hi - lo) / h + 2 * pad).astype(np.int64) + 1
    axes = [np.arange(int(d), dtype=np.float64) * h + float(o) for d, o in zip(dims, origin)]
    P = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    return origin, dims, P


def grad_S(S, iso, spacing, gV):
    """rule 6: gS (nx, ny, nz) fp32 for gV (n', 3) fp32; vertices past n' add nothing"""
    S = np.ascontiguousarray(S, dtype=F32)
    iso = np.float64(F32(iso))
    sp = _spacing3(spacing).astype(np.float64)
    gV = np.asarray(gV, dtype=F32).astype(np.float64)
    mask, offs = classify(S, iso)
    Sd = S.reshape(-1).astype(np.float64)
    acc = np.zeros(Sd.shape[0])
    node = np.arange(Sd.shape[0])
    terms = []
    for s in range(7):
        a = node[(mask >> s & 1) == 1]
        b = _edge_ends(S, s)[a]
        idx = _rank(mask, offs, a, s)
        keep = idx < gV.shape[0]
        a, b, idx = a[keep], b[keep], idx[keep]
        e = sp * SLOTS[s]
        g = gV[idx]
        ge = (g[:, 0] * e[0] + g[:, 1] * e[1]) + g[:, 2] * e[2]
        with np.errstate(all="ignore"):
            D = Sd[b] - Sd[a]
            t = (iso - Sd[a]) / D
            inside = (t >= 0) & (t <= 1)
            ta, tb = (-(1.0 - t) / D) * ge, (-t / D) * ge
        a, b, ta, tb = a[inside], b[inside], ta[inside], tb[inside]
        acc[a] += ta                                                   # a node owns at most one edge per slot: one add per node
        terms.append((b, tb))
    for b, tb in terms:
        acc[b] += tb
    return acc.astype(F32).reshape(S.shape)


# ---- the fp64 form: the positions of given grid edges as a smooth function of S, and its analytic gradient ---------------------------
def vertices64(S, iso, origin, spacing, E):
    S = np.asarray(S, dtype=np.float64)
    nx, ny, nz = S.shape
    Sf = S.reshape(-1)
    a, s = np.asarray(E) // 8, np.asarray(E) % 8
    d = SLOTS[s]
    ijk = np.stack(np.unravel_index(a, (nx, ny, nz)), 1)
    b = ((ijk[:, 0] + d[:, 0]) * ny + ijk[:, 1] + d[:, 1]) * nz + ijk[:, 2] + d[:, 2]
    t = (float(iso) - Sf[a]) / (Sf[b] - Sf[a])
    return np.asarray(origin, dtype=np.float64) + np.asarray(_spacing3(spacing), dtype=np.float64) * (ijk + t[:, None] * d)


def grad64(S, iso, spacing, E, gV):
    S = np.asarray(S, dtype=np.float64)
    nx, ny, nz = S.shape
    Sf = S.reshape(-1)
    a, s = np.asarray(E) // 8, np.asarray(E) % 8
    d = SLOTS[s]
    ijk = np.stack(np.unravel_index(a, (nx, ny, nz)), 1)
    b = ((ijk[:, 0] + d[:, 0]) * ny + ijk[:, 1] + d[:, 1]) * nz + ijk[:, 2] + d[:, 2]
    D = Sf[b] - Sf[a]
    t = (float(iso) - Sf[a]) / D
    ge = (np.asarray(gV, dtype=np.float64) * (np.asarray(_spacing3(spacing), dtype=np.float64) * d)).sum(1)
    g = np.zeros(Sf.shape[0])
    np.add.at(g, a, -(1.0 - t) / D * ge)
    np.add.at(g, b, -t / D * ge)
    return g.reshape(S.shape)


# ---- mesh properties the tests ask of a result ---------------------------------------------------------------------------------------
def directed_edges(F):
    F = np.asarray(F)
    return np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])


def boundary_edges(F):
    """the directed edges whose reverse does not appear, as (k, 2); raises if a directed edge appears twice"""
    de = directed_edges(F)
    n = int(de.max()) + 1 if de.size else 1
    key = de[:, 0] * n + de[:, 1]
    assert np.unique(key).size == key.size, "a directed edge appears twice"
    return de[~np.isin(key, de[:, 1] * n + de[:, 0])]


def euler(V, F):
    """V - E + F over the vertices the faces use"""
    de = np.sort(directed_edges(F), 1)
    return int(np.unique(F).size - np.unique(de, axis=0).shape[0] + F.shape[0])


def signed_volume(V, F):
    v = np.asarray(V, dtype=np.float64)
    return float(np.einsum("ij,ij->i", v[F[:, 0]], np.cross(v[F[:, 1]], v[F[:, 2]])).sum() / 6.0)


def grid_points(shape, origin=(0.0, 0.0, 0.0), spacing=1.0):
    """(nx, ny, nz, 3) fp64 node positions"""
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return np.asarray(origin, dtype=np.float64) + np.asarray(_spacing3(spacing), dtype=np.float64) * np.stack([i, j, k], -1)


def sphere_sdf(shape, centre, r, origin=(0.0, 0.0, 0.0), spacing=1.0):
    return (np.linalg.norm(grid_points(shape, origin, spacing) - np.asarray(centre, dtype=np.float64), axis=-1) - r).astype(F32)
