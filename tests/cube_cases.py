"""
Inputs of the cube-map tests (tests/test_cube_cpu.py, tests/test_cube_gpu.py, tests/test_cube_scale_gpu.py): directions built from
(face, texel-space position) through the face table read backwards, so that a test can say where on the cube its pixels land.
"""
import numpy as np

import cube_statement as cs


def direction(face, x, y, n, linear=True, length=1.0):
    """the direction whose lookup on an n x n cube lands at texel-space position (x, y) of `face` (linear: x = s n - 0.5, the position
    the taps are chosen by; nearest: x = s n), fp64 (..., 3)"""
    off = 0.5 if linear else 0.0
    face, x, y = np.broadcast_arrays(np.asarray(face), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    sc, tc = 2.0 * (x + off) / n - 1.0, 2.0 * (y + off) / n - 1.0
    return np.stack(cs._to_dir(face, sc, tc, np.ones_like(sc)), axis=-1) * np.asarray(length, dtype=np.float64)[..., None]


def directions_inside_cells(rng, n, linear, per_face=40, per_border=16):
    """fp64 directions (1, 1, P, 3) of random length whose texel-space coordinates keep 0.02 away from every integer (the kink of the
    bilinear lookup, the jump of the nearest one) and from the face's border: per face `per_face` random ones, and `per_border` within
    0.3 texels of its left / right borders, of its lower / upper borders and of its four corners -- every one of the 12 edges from both
    sides and every one of the 8 corners from three"""
    lo, hi = (-0.48, n - 0.52) if linear else (0.02, n - 0.02)

    def cell(size):
        c = rng.integers(0, n, size) + rng.uniform(0.02, 0.98, size)            # texel units, [0, n)
        return np.clip(c - 0.5 if linear else c, lo, hi)                         # linear: kinks at integer x = s n - 0.5

    def near(size):                 # within 0.3 texels of a border of the face, at either end
        u = rng.uniform(0.02, 0.3, size)
        return np.where(rng.random(size) < 0.5, u, n - u) - (0.5 if linear else 0.0)

    faces, xs, ys = [], [], []
    for f in range(6):
        for x, y in ((cell(per_face), cell(per_face)), (near(per_border), cell(per_border)), (cell(per_border), near(per_border)),
                     (near(per_border), near(per_border))):
            faces.append(np.full(x.shape, f)); xs.append(x); ys.append(y)
    f, x, y = np.concatenate(faces), np.concatenate(xs), np.concatenate(ys)
    return direction(f, x, y, n, linear, rng.uniform(0.5, 2.0, f.shape))[None, None]


# ---- threshold: clusters of pixels on single cells of an 8 x 8 cube; (items, face, i0, j0). The last two meet on the border texels
# (+x, i = 0, j = 3 .. 4): 40 items come across the edge from +z (whose taps at i = 8 fold there), 25 from +x itself -- 65 in all, past
# the 64 of one thread, only through the seam.
THRESHOLD_N = 8
THRESHOLD_CLUSTERS = [(63, 1, 2, 2), (64, 2, 2, 2), (65, 3, 2, 2), (129, 5, 4, 4), (1, 5, 1, 1), (40, 4, 7, 3), (25, 0, 0, 3)]


def threshold_directions(rng, linear):
    """fp32 (1, 1, P, 3), the clusters' pixels shuffled: the sort has work to do. Linear: a random offset in [0.1, 0.9) of the cell, so
    the four taps of a cluster's pixels are the same four texels; nearest: the centre of texel (i0, j0)"""
    d = []
    for m, f, i0, j0 in THRESHOLD_CLUSTERS:
        if linear:
            x, y = i0 + rng.uniform(0.1, 0.9, m), j0 + rng.uniform(0.1, 0.9, m)
            if i0 == THRESHOLD_N - 1:               # stay on the face: x <= n - 0.5
                x = i0 + rng.uniform(0.1, 0.45, m)
        else:
            x, y = np.full(m, i0 + 0.5), np.full(m, j0 + 0.5)
        d.append(direction(np.full(m, f), x, y, THRESHOLD_N, linear, rng.uniform(0.5, 2.0, m)))
    d = np.concatenate(d)
    return d[rng.permutation(len(d))].astype(np.float32)[None, None]
