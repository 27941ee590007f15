"""
Irregular meshes, CPU only (the native library is needed for the patch planner, no device): the helpers of tests/irregular_meshes.py keep
their promises -- the branch coverage of tests/test_row_kernels_gpu.py rests on them -- and the patch planner (csrc/patch_plan.cpp and its
numpy statement) is right for patches of every width class, W > 8 included, which no valence-6 mesh reaches.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import irregular_meshes as im
import patch_plan_statement as pps
from largesteps.patches import PatchPlan
from oracle import laplacian as ol
from statements import patch_steps

UP = (0.0, 0.0, 1.0)


def test_delaunay_sheet_keeps_its_promises():
    v, f = im.delaunay_sheet(4000, seed=0)
    assert v.dtype == np.float32 and f.dtype == np.int64 and v.shape == (4000, 3)
    im.check_manifold_oriented(v, f, up=UP)
    v2, f2 = im.delaunay_sheet(4000, seed=0)
    assert np.array_equal(v, v2) and np.array_equal(f, f2), "deterministic for a given seed"
    assert not np.array_equal(v, im.delaunay_sheet(4000, seed=1)[0])
    val = im.valence(4000, f)
    hist = np.bincount(val)
    assert val.min() >= 3 and val.max() >= 12 and (hist[4:11] > 0).all(), f"valences are spread: {hist}"
    w = im.sell_widths(val + 1)                        # a matrix row = the neighbours + the diagonal
    assert (w >= 9).all(), "every SELL-64 slice of a Delaunay mesh is wider than the unrolled form of row_sell"
    assert ((w >= 9) & (w <= 11)).any() and ((w > 8) & (w % 4 != 0)).any() and ((w > 8) & (w % 4 == 0)).any()
    assert (im.sell_widths(val) > 8).any()             # k_cheb_uniform's slices hold no diagonal


@pytest.mark.parametrize("n", [64, 100])
def test_planted_plane_keeps_its_promises(n):
    from largesteps import synthetic
    v, f, band = im.planted_plane(n)
    v0, f0 = synthetic.plane(n)
    assert np.array_equal(v, v0) and f.shape == f0.shape and f.dtype == np.int64, "flips move no vertex and keep the face count"
    im.check_manifold_oriented(v, f, up=UP)
    val = im.valence(n * n, f)
    assert np.array_equal(np.unique(band), np.arange(4))
    top = [int(val[band == b].max()) for b in range(4)]
    assert top[:3] == [6, 7, 8] and top[3] >= 12, f"maximum valence per band: {top}"
    for b in (1, 2, 3):
        assert (val[band == b] == top[b]).sum() >= 4, "several planted vertices per band"
    assert np.array_equal(np.bincount(val[band == 0]), np.bincount(im.valence(n * n, f0)[band == 0])), "band 0 is untouched"
    w = im.sell_widths(val + 1)
    assert (w <= 8).any() and ((w >= 9) & (w <= 11)).any() and ((w > 8) & (w % 4 != 0)).any(), f"SELL widths {np.bincount(w)}"


def test_hub_mesh_keeps_its_promises():
    v, f, hubs = im.hub_mesh(64, valences=(40, 300))
    V = v.shape[0]
    im.check_manifold_oriented(v, f, up=UP)
    val = im.valence(V, f)
    assert val[hubs].tolist() == [40, 300]
    rest = np.delete(val, hubs)
    assert rest.max() < 40 and np.bincount(rest).argmax() == 6 and (rest == 6).sum() > 0.8 * V, "a regular mesh but for the hubs"
    w = im.sell_widths(val + 1)
    assert w.max() == 301 and (w <= 8).any()


def test_csr_with_row_lengths_keeps_its_promises():
    lengths = np.array([0, 1, 7, 8, 9, 300, 17, 0, 3000] + [5] * 2991)
    M, A = im.csr_with_row_lengths(lengths, seed=3)
    V = lengths.shape[0]
    assert M.is_coalesced() and tuple(M.shape) == (V, V) and M.dtype.is_floating_point and A.dtype == np.float64
    idx, val = M.indices().numpy(), M.values().numpy()
    assert val.dtype == np.float32 and (val != 0).all()
    assert np.array_equal(np.bincount(idx[0], minlength=V), lengths), "exactly the requested row lengths"
    key = idx[0] * V + idx[1]
    assert (np.diff(key) > 0).all(), "distinct columns, row-major sorted"
    assert np.array_equal(A.indptr, im.csr_arrays(idx[0], V)) and np.array_equal(A.indices, idx[1]) and np.array_equal(A.data, val.astype(np.float64))
    M2, _ = im.csr_with_row_lengths(lengths, seed=3)
    assert np.array_equal(M2.values().numpy(), val) and np.array_equal(M2.indices().numpy(), idx)
    S, As = im.csr_with_row_lengths(np.full(500, 9), seed=1, symmetric=True)
    assert abs(As - As.T).max() == 0.0 and np.linalg.eigvalsh(As.toarray()).min() > 0.0
    assert np.array_equal(S.values().numpy().astype(np.float64), As.data)


# ---- the patch plan on patches of every width class -------------------------------------------------------------------------------
_SYSTEMS = {}


def _system(name):
    if name not in _SYSTEMS:
        v, f = im.planted_plane(64)[:2] if name == "planted" else im.delaunay_sheet(4000, seed=0)
        lam = 10.0
        r, c, val = ol.compute_matrix(v, f, lam)
        V = v.shape[0]
        rp = im.csr_arrays(r, V)
        A = sp.csr_matrix((val.astype(np.float64), c, rp), shape=(V, V))
        b = A @ v.astype(np.float64)
        n, c1, c2 = im.chebyshev_schedule(A, 1.0, 1e-6)
        d = A.diagonal()
        xc, xp = np.zeros_like(b), np.zeros_like(b)
        for it in range(n):                              # the global iteration, computed once per mesh
            xc, xp = xc + c1[it] * (xc - xp) + c2[it] * (b - A @ xc) / d[:, None], xc
        _SYSTEMS[name] = (v, lam, rp, c, A, b, (n, c1, c2), xc)
    return _SYSTEMS[name]


# which width classes the patches of each mesh must reach: the planted plane all four at once, the Delaunay sheet (no patch of ~100
# random vertices is free of a vertex of valence 9) the form no regular mesh reaches
_CLASSES = {"planted": {"<=6", "7", "8", ">8"}, "delaunay": {">8"}}


@pytest.mark.parametrize("impl", ["native", "statement"])
@pytest.mark.parametrize("name", ["planted", "delaunay"])
@pytest.mark.parametrize("patch_size,depth", [(128, 2), (256, 4)])
def test_patch_plan_reproduces_global_iteration_for_every_width(name, patch_size, depth, impl):
    v, lam, rp, c, A, b, (n, c1, c2), xc = _system(name)
    V = v.shape[0]
    d = A.diagonal()
    build = PatchPlan.build if impl == "native" else pps.PatchPlan.build
    plan = build(rp, c, d, v, patch_size=patch_size, depth=depth, cap_local=6000)
    assert plan is not None and plan.depth == depth
    T = plan.table
    assert T[0, 0] == 0 and (T[1:, 0] == T[:-1, 0] + T[:-1, 1]).all() and T[-1, 0] + T[-1, 1] == V
    assert T[:, 1].max() <= patch_size and plan.max_local < 65535
    assert sorted(plan.perm.tolist()) == list(range(V))
    assert (plan.cols16.astype(np.int64).reshape(-1) <= plan.max_local).all()
    assert plan.redundancy < 4.0
    assert im.width_classes(T[:, 4]) >= _CLASSES[name], f"patch widths {np.bincount(T[:, 4])}"
    assert plan.max_width == T[:, 4].max() == im.valence(V, _faces(name)).max()
    # a patch's width is the longest of ITS rows, and its ELL block lists exactly the neighbours of every row
    val_new = (np.diff(rp) - 1)[plan.perm]
    for row in T:
        own_start, n_own, n_rows, n_local, W, og, oc = (int(t) for t in row[:7])
        gid = np.concatenate([np.arange(own_start, own_start + n_own), plan.ghost_gid[og:og + n_local - n_own]])
        assert W == val_new[gid[:n_rows]].max()
        ell = plan.cols16[oc:oc + W * n_rows].reshape(W, n_rows).astype(np.int64)
        assert np.array_equal((ell < n_local).sum(axis=0), val_new[gid[:n_rows]])
    bn = b[plan.perm]
    cur, prev = np.zeros_like(b), np.zeros_like(b)
    for it0 in range(0, n, plan.depth):
        cur, prev = patch_steps(plan, -lam, bn, cur, prev, c1[it0:it0 + plan.depth], c2[it0:it0 + plan.depth])
    x = np.empty_like(cur)
    x[plan.perm] = cur
    assert np.abs(x - xc).max() <= 1e-12 * np.abs(xc).max(), "s steps on overlapping patches == s global steps"
    assert np.abs(x - v).max() <= 1e-5


def _faces(name):
    return im.planted_plane(64)[1] if name == "planted" else im.delaunay_sheet(4000, seed=0)[1]


@pytest.mark.parametrize("name", ["planted", "delaunay"])
def test_native_patch_plan_equals_its_statement_on_irregular_rows(name):
    """Same patches, same ghost layers, same ELL ids: the two planners are compared array by array where their orders are defined
    (the cut into patches; inside a patch both sort by the same keys)."""
    v, lam, rp, c, A = _system(name)[:5]
    d = A.diagonal()
    a = PatchPlan.build(rp, c, d, v, patch_size=128, depth=3, cap_local=6000)
    s = pps.PatchPlan.build(rp, c, d, v, patch_size=128, depth=3, cap_local=6000)
    assert a.depth == s.depth and a.n_patches == s.n_patches
    assert np.array_equal(np.sort(a.table[:, 4]), np.sort(s.table[:, 4])), "the same multiset of patch widths"
    assert a.max_width == s.max_width and a.max_rows == s.max_rows and a.max_local == s.max_local


def test_native_patch_plan_on_irregular_rows_is_independent_of_the_thread_count(monkeypatch):
    v, lam, rp, c, A = _system("planted")[:5]
    d = A.diagonal().astype(np.float32)
    plans = []
    for t in ("1", "3", "8"):
        monkeypatch.setenv("LS_PLAN_THREADS", t)
        plans.append(PatchPlan.build(rp, c, d, v, patch_size=128, depth=3, cap_local=6000))
    assert im.width_classes(plans[0].table[:, 4]) == _CLASSES["planted"]
    for q in plans[1:]:
        for name in ("perm", "table", "ghost_gid", "cols16", "diag"):
            assert np.array_equal(getattr(plans[0], name), getattr(q, name)), name
