"""
Meshes and matrices with IRREGULAR rows (TEST code, numpy / scipy only, deterministic for a given seed).

Every synthetic mesh of largesteps.synthetic has valence 6 at most, so a row of its system matrix has at most 7 entries, a SELL-64
slice is at most 7 wide and a 256-row tile holds at most 1792 entries: the kernels' branches for longer rows never run on them. The
helpers below build what does reach those branches:

    delaunay_sheet(n, seed)        Delaunay triangulation of random points: valences spread over 3 .. ~15, every SELL slice wider than 8
    planted_plane(n)               synthetic.plane(n) with four spatial bands of maximum valence exactly 6, exactly 7, exactly 8 and >= 12
                                   (edge flips that keep the mesh manifold and oriented): all four width classes of the patch kernel at once
    hub_mesh(n, valences)          a regular lattice with single vertices of valence exactly 40 and exactly 300
    csr_with_row_lengths(...)      a foreign matrix with prescribed row lengths (any length, 0 included)

and the numpy counterparts of what the tests assert about them (valence, manifoldness, SELL-64 widths).
"""
import numpy as np
import scipy.sparse as sp
import torch

from largesteps import synthetic


# ---- measurements -------------------------------------------------------------------------------------------------------
def valence(V, f):
    """number of distinct neighbours of every vertex (= off-diagonal row length of the mesh Laplacian)"""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    return np.bincount(e.reshape(-1), minlength=V)


def check_manifold_oriented(v, f, up=None):
    """Edge-manifold with consistent orientation: every directed edge occurs once, every undirected edge in at most two faces (then
    once per direction), no degenerate face, every vertex's faces form ONE fan, and (up given) every face normal points along `up`
    (the meshes here are height fields, so the orientation of synthetic.plane is kept face by face). Raises AssertionError."""
    V = v.shape[0]
    assert f.dtype == np.int64 and f.min() >= 0 and f.max() < V
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * V + d[:, 1]
    assert np.unique(key).shape[0] == key.shape[0], "a directed edge occurs twice: not manifold or not consistently oriented"
    # one fan per vertex: faces around a vertex = its valence (interior) or valence - 1 (boundary), and a boundary vertex has
    # exactly two boundary edges
    rev = d[:, 1] * V + d[:, 0]
    boundary = ~np.isin(key, rev)
    nb = np.bincount(d[boundary].reshape(-1), minlength=V)
    assert set(np.unique(nb).tolist()) <= {0, 2}, "a vertex with more than one boundary fan"
    fan = np.bincount(f.reshape(-1), minlength=V)
    val = valence(V, f)
    used = fan > 0
    assert (fan[used] == val[used] - (nb[used] > 0)).all(), "a vertex whose faces are not one fan"
    p = v.astype(np.float64)
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert (np.linalg.norm(n, axis=1) > 0).all(), "degenerate face"
    if up is not None:
        assert (n @ np.asarray(up, dtype=np.float64) > 0).all(), "a face changed its orientation"


def sell_widths(row_lengths, height=64):
    """width of every SELL slice of `height` rows: the longest row of the slice (csrc/pcg.hip k_sell_widths)"""
    n = np.asarray(row_lengths, dtype=np.int64)
    pad = (-n.shape[0]) % height
    return np.concatenate([n, np.zeros(pad, np.int64)]).reshape(-1, height).max(axis=1)


def tile_entries(row_lengths, rows=256):
    """entries of every 256-row tile of the CSR product (csrc/spmv_kernels.h row_csr_lds stages a tile of <= LDS_CAP entries)"""
    n = np.asarray(row_lengths, dtype=np.int64)
    pad = (-n.shape[0]) % rows
    return np.concatenate([n, np.zeros(pad, np.int64)]).reshape(-1, rows).sum(axis=1)


# ---- Delaunay sheet -------------------------------------------------------------------------------------------------------
def _height(x, y):
    return 0.1 * np.sin(2.0 * np.pi * x) * np.cos(2.0 * np.pi * y)


def delaunay_sheet(n, seed=0):
    """Delaunay triangulation of n uniform random points of the unit square, lifted by a smooth height function; faces
    counter-clockwise seen from +z. Returns (float32 vertices (n,3), int64 faces). The vertex order is the random one of the
    points: rows of very different length share every SELL slice and every tile."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    p = rng.random((n, 2))
    f = Delaunay(p).simplices.astype(np.int64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    f[area2 < 0] = f[area2 < 0][:, [0, 2, 1]]
    v = np.stack([p[:, 0], p[:, 1], _height(p[:, 0], p[:, 1])], axis=1).astype(np.float32)
    return v, f


# ---- edge flips on a height field -------------------------------------------------------------------------------------------
class _Flipper:
    """Triangle mesh over the xy plane with the half-edge table an edge flip needs. A flip is accepted only if it keeps the mesh a
    manifold (the new edge does not exist yet, no valence drops below `min_valence`, no boundary edge) and keeps both new faces
    counter-clockwise with a real area (the quadrilateral is strictly convex)."""

    def __init__(self, v, f, min_valence=4):
        self.p = v[:, :2].astype(np.float64)
        self.f = [list(map(int, t)) for t in f]
        self.he = {}
        for i, (a, b, c) in enumerate(self.f):
            self.he[(a, b)] = i
            self.he[(b, c)] = i
            self.he[(c, a)] = i
        self.vf = [set() for _ in range(v.shape[0])]
        for i, t in enumerate(self.f):
            for a in t:
                self.vf[a].add(i)
        self.val = valence(v.shape[0], f).astype(np.int64)
        self.min_valence = min_valence
        scale = np.abs(self.p[f[:, 1]] - self.p[f[:, 0]]).max()
        self.min_area2 = 0.25 * scale * scale          # (a unit cell of the grid has area2 = scale^2 / 2 per triangle)

    def _area2(self, a, b, c):
        p = self.p
        return (p[b, 0] - p[a, 0]) * (p[c, 1] - p[a, 1]) - (p[b, 1] - p[a, 1]) * (p[c, 0] - p[a, 0])

    def third(self, a, b):
        i = self.he.get((a, b))
        if i is None:
            return None
        t = self.f[i]
        return t[(t.index(a) + 2) % 3]

    def link(self, v):
        """the directed edges (p, q) opposite to v, one per face (v, p, q)"""
        out = []
        for i in sorted(self.vf[v]):
            t = self.f[i]
            k = t.index(v)
            out.append((t[(k + 1) % 3], t[(k + 2) % 3]))
        return out

    def flip(self, a, b, allowed=None, cap=None):
        """faces (a, b, c), (b, a, d) -> (a, d, c), (d, b, c); returns d or None (refused)"""
        c, d = self.third(a, b), self.third(b, a)
        if c is None or d is None or (c, d) in self.he or (d, c) in self.he:
            return None
        if self.val[a] - 1 < self.min_valence or self.val[b] - 1 < self.min_valence:
            return None
        if allowed is not None and not (allowed[a] and allowed[b] and allowed[d]):
            return None
        if cap is not None and self.val[d] + 1 > cap:
            return None
        if self._area2(a, d, c) < self.min_area2 or self._area2(d, b, c) < self.min_area2:
            return None
        i, j = self.he.pop((a, b)), self.he.pop((b, a))
        self.f[i], self.f[j] = [a, d, c], [d, b, c]
        self.he[(a, d)] = self.he[(d, c)] = self.he[(c, a)] = i
        self.he[(d, b)] = self.he[(b, c)] = self.he[(c, d)] = j
        self.vf[b].discard(i), self.vf[d].add(i), self.vf[a].discard(j), self.vf[c].add(j)
        self.val[a] -= 1
        self.val[b] -= 1
        self.val[c] += 1
        self.val[d] += 1
        return d

    def raise_valence(self, v, target, allowed=None, cap=None):
        """flip the edge opposite to v, nearest candidate first, until v has `target` neighbours; False if it got stuck (on a grid
        the vertex behind a link edge is sooner or later hidden behind one of the edge's ends: ~12 is what plain flips reach)"""
        while self.val[v] < target:
            cand = []
            for (p, q) in self.link(v):
                d = self.third(q, p)
                if d is not None:
                    cand.append((float(((self.p[d] - self.p[v]) ** 2).sum()), p, q))
            for _, p, q in sorted(cand):
                if self.flip(p, q, allowed, cap) is not None:
                    break
            else:
                return False
        return True

    def faces(self):
        return np.asarray(self.f, dtype=np.int64)


BAND_TARGETS = (6, 7, 8, 12)       # maximum valence of the four bands of planted_plane: exactly 6, 7, 8; at least 12


def planted_plane(n, margin=6, spacing=(5, 5, 9)):
    """synthetic.plane(n) cut into four bands of rows (y quarters). Band 0 is untouched (maximum valence exactly 6); in bands 1, 2, 3 a
    lattice of vertices, `margin` rows away from the band's borders, is raised to valence 7, 8 and 12 by flipping the edges opposite to
    it, and no other vertex of the band may exceed 7, 8 (band 3: no bound). Returns (v, f, band): the band of every vertex."""
    v, f = synthetic.plane(n)
    rows = np.arange(n * n) // n
    cols = np.arange(n * n) % n
    edges = [0, n // 4, n // 2, (3 * n) // 4, n]
    band = np.searchsorted(np.asarray(edges[1:]), rows, side="right").astype(np.int64)
    m = _Flipper(v, f)
    for b in (1, 2, 3):
        lo, hi = edges[b], edges[b + 1]
        inside = (band == b) & (rows >= lo + 2) & (rows < hi - 2) & (cols >= 2) & (cols < n - 2)
        step = spacing[b - 1]
        for y in range(lo + margin, hi - margin, step):
            for x in range(margin, n - margin, step):
                ok = m.raise_valence(y * n + x, BAND_TARGETS[b], allowed=inside, cap=None if b == 3 else BAND_TARGETS[b])
                assert ok, f"planted_plane: vertex ({x}, {y}) of band {b} could not reach valence {BAND_TARGETS[b]}"
    return v, m.faces(), band


def hub_mesh(n=64, valences=(40, 300), at=((0.3, 0.25), (0.7, 0.6)), radius=(0.05, 0.12)):
    """A regular (equilateral, valence 6) lattice of ~n x n vertices over the unit square in which one vertex per entry of `valences`
    has exactly that valence: the 'one vertex of very high valence' of a scanned mesh. Around hub i (at[i] = (x, y)) the lattice is
    cleared inside radius[i] and valences[i] vertices are put on that circle; the Delaunay triangulation then joins the hub to every
    one of them and to nothing else (the circle through the hub and two neighbours of the ring stays inside the cleared disc).
    Returns (v, f, hubs)."""
    from scipy.spatial import Delaunay
    h = 1.0 / (n - 1)
    j, i = np.meshgrid(np.arange(int(round((n - 1) / (0.5 * 3 ** 0.5))) + 1), np.arange(n), indexing="ij")
    p = np.stack([(i + 0.5 * (j % 2)) * h, j * h * (0.5 * 3 ** 0.5)], axis=-1).reshape(-1, 2)
    p = p[(p[:, 0] <= 1.0 + 0.25 * h) & (p[:, 1] <= 1.0 + 0.25 * h)]
    extra = []
    for t, c, r in zip(valences, at, radius):
        c = np.asarray(c, dtype=np.float64)
        p = p[np.linalg.norm(p - c, axis=1) > r + 0.5 * h]
        ang = 2.0 * np.pi * (np.arange(t) + 0.25) / t
        extra += [c[None, :], c + r * np.stack([np.cos(ang), np.sin(ang)], axis=1)]
    hubs = p.shape[0] + np.concatenate([[0], np.cumsum([e.shape[0] for e in extra])])[0:-1:2]
    p = np.concatenate([p] + extra)
    f = Delaunay(p).simplices.astype(np.int64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    f = f[np.abs(area2) > 1e-9 * h * h]            # (collinear lattice vertices of the hull can give a flat face)
    area2 = area2[np.abs(area2) > 1e-9 * h * h]
    f[area2 < 0] = f[area2 < 0][:, [0, 2, 1]]
    v = np.stack([p[:, 0], p[:, 1], _height(p[:, 0], p[:, 1])], axis=1).astype(np.float32)
    return v, f, hubs.astype(np.int64)


# ---- foreign matrices -------------------------------------------------------------------------------------------------------
def csr_with_row_lengths(lengths, V=None, seed=0, symmetric=False, device=None):
    """A (V, V) matrix whose row i has exactly lengths[i] entries in random distinct columns, values uniform in [-1, 1] (fp32, never
    zero). symmetric=True returns A + A^T + a dominant diagonal instead (SPD; the row lengths are then only approximately the
    requested ones). Returns (coalesced torch.sparse_coo_tensor on `device`, scipy fp64 CSR with the same entries in the same order)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    V = int(lengths.shape[0]) if V is None else int(V)
    assert lengths.shape[0] == V and (lengths <= V).all() and (lengths >= 0).all()
    rng = np.random.default_rng(seed)
    cols = []
    for n in lengths:
        if n == 0:
            cols.append(np.empty(0, np.int64))
        elif 4 * n < V:
            c = np.unique(rng.integers(0, V, size=int(n)))
            while c.shape[0] < n:
                c = np.unique(np.concatenate([c, rng.integers(0, V, size=int(n - c.shape[0]))]))
            cols.append(c)
        else:
            cols.append(np.sort(rng.permutation(V)[:n]))
    col = np.concatenate(cols) if cols else np.empty(0, np.int64)
    row = np.repeat(np.arange(V, dtype=np.int64), lengths)
    val = rng.uniform(0.05, 1.0, size=col.shape[0]) * rng.choice([-1.0, 1.0], size=col.shape[0])
    A = sp.csr_matrix((val.astype(np.float32), (row, col)), shape=(V, V))
    if symmetric:
        A = (A + A.T).tocsr()
        A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).reshape(-1) + 1.0)).tocsr().astype(np.float32)
    A.sort_indices()
    return coo_of(A, device), A.astype(np.float64)


def coo_of(A, device=None):
    """the coalesced torch COO matrix (fp32) of a scipy CSR matrix with sorted indices"""
    coo = A.tocoo()            # row-major, columns ascending: the coalesced order
    idx = torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64))
    M = torch.sparse_coo_tensor(idx, torch.from_numpy(coo.data.astype(np.float32)), A.shape)
    if device is not None:
        M = M.to(device)
    return M.coalesce()


# ---- systems ------------------------------------------------------------------------------------------------------------------
def csr_arrays(rows, V):
    """rowptr of sorted COO rows"""
    rp = np.zeros(V + 1, np.int64)
    np.add.at(rp, np.asarray(rows) + 1, 1)
    return np.cumsum(rp)


def chebyshev_schedule(A, a_min, reduction):
    """(n, c1, c2): step count and coefficients of the Chebyshev-Jacobi iteration of csrc/pcg.hip solve_cheb for the fp64 matrix A:
    enclosure [0.98 a_min / max diag, Gershgorin (1 + 1e-5)] of spec(D^-1 A), n from the requested residual reduction."""
    import math
    d = A.diagonal()
    lmax = (np.asarray(abs(A).sum(axis=1)).reshape(-1) / d).max() * (1 + 1e-5)
    lmin = 0.98 * a_min / d.max()
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma1 = theta / delta
    sk = math.sqrt(lmax / lmin)
    n = int(math.ceil(math.log(2 / reduction) / -math.log((sk - 1) / (sk + 1))))
    c1, c2, rho = [], [], 1 / sigma1
    for it in range(n):
        if it == 0:
            c1.append(0.0), c2.append(1 / theta)
        else:
            rn = 1 / (2 * sigma1 - rho)
            c1.append(rn * rho), c2.append(2 * rn / delta)
            rho = rn
    return n, c1, c2


def width_classes(widths):
    """which of the patch kernel's four forms (csrc/pcg.hip k_patch_cheb: W <= 6, == 7, == 8 in registers, > 8 re-read) a set of
    patch widths reaches"""
    w = np.asarray(widths)
    return {name for name, hit in (("<=6", (w <= 6).any()), ("7", (w == 7).any()), ("8", (w == 8).any()), (">8", (w > 8).any())) if hit}
