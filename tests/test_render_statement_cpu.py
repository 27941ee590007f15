"""
tests/render_statement_fast.py (vectorised, used at production shapes by tests/test_render_scale_gpu.py) against tests/render_statement.py
(the loop specification): id maps, u, v, z/w and every fp32 output bitwise, fp64 gradients to 1e-12 of the sum of their terms' absolute
values. No device needed.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import render_statement as rs  # noqa: E402
import render_statement_fast as rf  # noqa: E402
from render_scenes import SCENES, grid_mesh, near_plane_triangles, random_soup, scene  # noqa: E402


def _scene(name):
    if name.startswith("soup"):
        return random_soup(int(name[4:]))
    if name.startswith("grid"):
        seed = int(name[4:])
        pos, f = grid_mesh(9, -1.25, 1.25, jitter=0.12, seed=seed, wscale=seed > 0)
        return pos, f, 24, 32
    if name == "centres":
        W = H = 16
        c = rs.centres(W)
        n = W // 2 + 3
        pos, f = grid_mesh(n, 0, 0, coords=c[0] + (c[1] - c[0]) * (2 * np.arange(n) - 2))
        return pos, f, H, W
    if name == "near_tris":                       # the random near-plane triangles as one mesh (they overlap: depth decides)
        q = near_plane_triangles()
        return np.concatenate(q)[None], np.arange(3 * len(q)).reshape(-1, 3), 24, 24
    return scene(name)


ALL = SCENES + ["sheet", "grid0", "grid1", "grid2", "centres", "near_tris", "soup0", "soup1", "soup2"]


def _close(a, b, ab):
    """fp64 results of two summation orders: within 1e-12 of the sum of the absolute values of the terms"""
    err = np.abs(np.asarray(a, np.float64) - b)
    assert np.all(err <= 1e-12 * ab + 1e-300), float((err / np.maximum(ab, 1e-300)).max())


@pytest.mark.parametrize("name", ALL)
def test_fast_statement_equals_loop_statement(name):
    pos, f, H, W = _scene(name)
    B, V = pos.shape[0], pos.shape[1]
    rng = np.random.default_rng(5)
    r = rf.rasterize(pos, f, H, W, chunk=97)               # small chunks: the chunk boundaries are exercised too
    rl = rs.rasterize(pos, f, H, W)
    assert np.array_equal(r.view(np.uint32), rl.view(np.uint32))
    assert np.array_equal(rf.adjacency(f), rs.adjacency(f))
    attr = rng.uniform(-1, 1, (1, V, 3)).astype(np.float32)
    col = rf.interpolate(attr, r, f)
    assert np.array_equal(col.view(np.uint32), rs.interpolate(attr, r, f).view(np.uint32))
    aa = rf.antialias(col, r, pos, f)
    assert np.array_equal(aa.view(np.uint32), rs.antialias(col, r, pos, f).view(np.uint32))
    g = rng.standard_normal(col.shape).astype(np.float32)
    gc, gp, agc, agp, _, _ = rf.antialias_backward(col, r, pos, f, g, boost=1.5)
    gcl, gpl = rs.antialias_backward(col, r, pos, f, g, boost=1.5)
    _close(gc, gcl, agc)
    _close(gp, gpl, agp)
    ga, gr, aga, agr = rf.interpolate_backward(attr, r, f, g)
    gal, grl = rs.interpolate_backward(attr, r, f, g)
    _close(ga, gal, aga)
    _close(gr, grl, agr)
    gq = rng.standard_normal(r.shape).astype(np.float32)
    gpr, agpr = rf.rasterize_backward(pos, f, r, gq, chunk=101)
    _close(gpr, rs.rasterize_backward(pos, f, r, gq), agpr)
    assert np.all(gpr[..., 2] == 0) and np.all(gp[..., 2] == 0)
    if name.startswith("soup"):                                # the random soups are what they claim to be
        assert (pos[..., 3] <= 0).mean() > 0.15
        assert (rf.adjacency(f) == -1).sum() > 0
        assert len(np.unique(np.sort(f, 1), axis=0)) < len(f)


@pytest.mark.parametrize("attr_batch", [1, 3])
def test_fast_interpolate_backward_batches(attr_batch):
    pos, f, H, W = scene("sphere_b3")
    B, V = pos.shape[0], pos.shape[1]
    rng = np.random.default_rng(6)
    r = rf.rasterize(pos, f, H, W)
    attr = rng.uniform(-1, 1, (attr_batch, V, 5)).astype(np.float32)
    col = rf.interpolate(attr, r, f)
    assert np.array_equal(col, rs.interpolate(attr, r, f))
    g = rng.standard_normal(col.shape).astype(np.float32)
    ga, gr, aga, agr = rf.interpolate_backward(attr, r, f, g)
    gal, grl = rs.interpolate_backward(attr, r, f, g)
    _close(ga, gal, aga)
    _close(gr, grl, agr)


def test_adjacency_marks_non_manifold_and_boundary_edges():
    # two triangles on edge (0, 1), three on edge (2, 3), a lone face
    f = np.array([[0, 1, 2], [1, 0, 4], [2, 3, 5], [3, 2, 6], [2, 3, 7], [8, 9, 10]])
    adj = rf.adjacency(f)
    assert np.array_equal(adj, rs.adjacency(f))
    assert adj[0, 0] == 1 and adj[1, 0] == 0
    assert np.all(adj[2:5, 0] == -1) and np.all(adj[5] == -1)


def test_summation_depth():
    m = np.array([[0, 1, 64, 65, 128, 129, 10 ** 6]])
    assert rf.seg_depth(m).tolist() == [[0, 1, 64, 8, 8, 9, 15631]]
    assert rf.seg_depth(m, terms=np.array([[0, 3, 200, 70, 400, 2, 10]])).tolist() == [[0, 3, 200, 14, 14, 8, 16]]
    f = np.array([[0, 1, 2], [0, 2, 3]])
    d = rf.vertex_depth(np.array([[5, 70], [1, 2]]), f, 5)
    assert d.tolist() == [[72, 6, 72, 71, 0], [4, 2, 4, 3, 0]]
    assert rf.vertex_depth(np.array([[5, 70], [1, 2]]), f, 5, batches_summed=True).tolist() == [74, 7, 74, 72, 0]
