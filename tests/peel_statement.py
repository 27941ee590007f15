"""
Numpy statement of depth peeling (largesteps.render.DepthPeeler; csrc/raster.hip), built on the coverage rule and
the depth key of render_statement.py. It is the specification:

    for each image and pixel, collect every covering fragment (face f with z/w rounded to fp32 = zf); sort them by the key
    (order bits of zf) << 32 | f; layer l is the l-th of them, written (u, v, z/w, f + 1) as render_statement.rasterize writes the
    nearest one -- and zeros where the pixel has fewer than l + 1 fragments.

Layer 0 is render_statement.rasterize. Nothing here knows about "the previous layer": that the kernel's rule (the smallest key strictly
above the previous layer's) peels exactly these layers is what the tests check.
"""
import numpy as np

import render_statement as rs

F32 = np.float32
NONE = np.iinfo(np.uint64).max


def fragment_keys(pos_b, tri, H, W):
    """(F, H, W) uint64: the depth key of face f at each pixel of one image (pos_b (V, 4) fp32), NONE where f does not cover it"""
    pos_b = np.asarray(pos_b, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    py, px = np.meshgrid(rs.centres(H), rs.centres(W), indexing="ij")
    keys = np.full((tri.shape[0], H, W), NONE, dtype=np.uint64)
    for f in range(tri.shape[0]):
        m, _, zf = rs.cover(pos_b[tri[f]], px, py)
        if m.any():
            keys[f] = np.where(m, (rs._order_bits(zf) << np.uint64(32)) | np.uint64(f), NONE)
    return keys


def depth_complexity(pos, tri, H, W):
    """(B, H, W) int: the number of covering fragments of each pixel"""
    pos = np.asarray(pos, dtype=F32)
    return np.stack([(fragment_keys(pos[b], tri, H, W) != NONE).sum(0) for b in range(pos.shape[0])])


def _write(pos_b, tri, H, W, best):
    """the rast (H, W, 4) of the fragments whose keys are `best` (H, W), as render_statement.rasterize resolves its minimum"""
    py, px = np.meshgrid(rs.centres(H), rs.centres(W), indexing="ij")
    rast = np.zeros((H, W, 4), dtype=F32)
    hit = best != NONE
    ids = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for f in np.unique(ids[hit]):
        m = hit & (ids == f)
        _, E, zf = rs.cover(pos_b[tri[f]], px[m], py[m])
        S = (E[0] + E[1]) + E[2]
        rast[m] = np.stack([(E[0] / S).astype(F32), (E[1] / S).astype(F32), zf, np.full(m.sum(), f + 1, F32)], axis=-1)
    return rast


def peel(pos, tri, H, W, layers=None):
    """pos (B, V, 4) fp32, tri (F, 3) -> (L, B, H, W, 4) fp32: layers 0 .. L - 1. L = `layers`, or the largest depth complexity (so the
    last layer returned is the last non-empty one; at least 1)"""
    pos = np.asarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    B = pos.shape[0]
    ordered = [np.sort(fragment_keys(pos[b], tri, H, W), axis=0) for b in range(B)]
    if layers is None:
        layers = max([1] + [int((k != NONE).sum(0).max()) for k in ordered if k.shape[0]])
    out = np.zeros((layers, B, H, W, 4), dtype=F32)
    for b in range(B):
        for l in range(min(layers, ordered[b].shape[0])):
            out[l, b] = _write(pos[b], tri, H, W, ordered[b][l])
    return out


def layer_keys(rast):
    """the depth key each pixel of a rast (..., 4) was resolved by, NONE for background"""
    rast = np.asarray(rast, dtype=F32)
    ids = rast[..., 3].astype(np.int64)
    key = (rs._order_bits(rast[..., 2]) << np.uint64(32)) | (np.maximum(ids, 1) - 1).astype(np.uint64)
    return np.where(ids > 0, key, NONE)
