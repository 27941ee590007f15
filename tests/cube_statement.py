"""
The cube-map lookup of largesteps.render.texture(..., boundary_mode='cube'), stated in vectorised numpy (the yardstick of
tests/test_cube_cpu.py, tests/test_cube_gpu.py and tests/test_cube_scale_gpu.py; nvdiffrast's cube mode without mipmaps, written from the
contract and not from the kernel).

tex (Bt, 6, n, n, C) with Bt in {1, B}, faces +x, -x, +y, -y, +z, -z; uv (B, H, W, 3): a direction d = (x, y, z), any length.

    face      major axis: x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z; the face is the major axis' sign.
              (sc, tc, ma) = (-z, -y, x) (z, -y, x) (x, z, y) (x, -z, y) (x, -y, z) (-x, -y, z) for faces 0 .. 5;
              s = (sc / |ma| + 1) * 0.5, t = (tc / |ma| + 1) * 0.5: a division, an add, a multiply, in the coordinate type.
              A direction with a non-finite component, or (0, 0, 0), gives output 0 and no gradient.
    nearest   the texel (min(floor(s n), n - 1), min(floor(t n), n - 1)) of the face
    linear    x = s n - 0.5, i0 = floor(x) (clamped to [-1, n - 1]), fx = x - floor(x), likewise j0, fy; taps (i0 + dx, j0 + dy), tap id
              2 dy + dx, weight (fx or 1 - fx)(fy or 1 - fy)
    seams     a tap with exactly one index out of range (-1 or n): the centre of that texel on the extended plane of its face (|ma| = 1,
              sc or tc = +-(1 + 1 / n)) is a direction; the tap reads the texel a NEAREST lookup of that direction finds (`_fold`)
    corners   a tap with both indices out of range has no texel; its weight w_c goes to the other three, w'_k = w_k + w_c / 3
    out       no dropped tap: top + (bot - top) fy, top = t00 + (t10 - t00) fx, bot = t01 + (t11 - t01) fx; else sum of w'_k t_k
    grad_tex  w'_k g per (pixel, tap); a dropped tap contributes nothing
    grad_uv   linear only, the face choice held fixed: through the weights (the w_c / 3 terms included -- the same as a bilinear lookup
              whose missing texel is the mean of the other three) and the chain (s, t) -> d

Coordinates and fractions are computed in `coords` (np.float32: exactly the numbers the device uses; np.float64: for finite
differences); everything after them in fp64. Every returned sum comes with the sum of the absolute values of the terms that were added
and their number, for the error bounds of the device tests.
"""
from types import SimpleNamespace

import numpy as np

from texture_statement import _scatter

FILTERS = ("nearest", "linear")


def _to_dir(face, sc, tc, ma):
    """(sc, tc, ma) of `face` -> (x, y, z): the table read backwards (a signed permutation, so it carries gradients too)"""
    x = np.choose(face, [ma, -ma, sc, sc, sc, -sc])
    y = np.choose(face, [-tc, -tc, ma, -ma, -tc, -tc])
    z = np.choose(face, [-sc, sc, tc, -tc, ma, -ma])
    return x, y, z


def _face(d, coords):
    """directions (..., 3) of type `coords` -> finite, face, sc / |ma|, tc / |ma|, |ma| (the last three in `coords`)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ((ax > 0) | (ay > 0) | (az > 0))
        a = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
        ma = np.choose(a, [x, y, z])
        face = 2 * a + (ma < 0)
        sc = np.choose(face, [-z, z, x, x, x, -x])
        tc = np.choose(face, [-y, -y, z, -z, -y, -y])
        ama = np.abs(ma)
        qs = np.where(finite, sc / ama, 0).astype(coords)
        qt = np.where(finite, tc / ama, 0).astype(coords)
    return finite, np.where(finite, face, 0), qs, qt, np.where(finite, ama, 1).astype(coords)


def _nearest_texel(d, n, coords):
    """directions (..., 3) -> finite, face, i, j of the texel that contains them"""
    finite, face, qs, qt, _ = _face(d, coords)
    s, t = (qs + coords(1)) * coords(0.5), (qt + coords(1)) * coords(0.5)
    i = np.clip(np.floor(s * coords(n)), 0, n - 1).astype(np.int64)
    j = np.clip(np.floor(t * coords(n)), 0, n - 1).astype(np.int64)
    return finite, face, i, j


def _fold(face, i, j, n):
    """texel (i, j) of `face` with exactly one index out of range -> (face, i, j) of the neighbour's texel that contains the centre of the
    out-of-range texel, taken on the extended plane of its face"""
    sc, tc = (2.0 * i + 1.0) / n - 1.0, (2.0 * j + 1.0) / n - 1.0
    d = np.stack(_to_dir(face, sc, tc, np.ones_like(sc)), axis=-1)
    _, f2, i2, j2 = _nearest_texel(d, n, np.float64)
    return f2, i2, j2


def cube(tex, uv, g=None, filter_mode="linear", coords=np.float32):
    """
    Returns a namespace with
        out, out_abs (B, H, W, C)                       the lookup and the sum of |weight * texel| over its taps
        face, i0, j0 (B, H, W) int64, finite (B, H, W) bool   the face and the base tap (nearest: the texel)
        drop (B, H, W) int64                            the tap without a texel, -1 for none
        inside (B, H, W) bool                           all four taps lie inside the face
    and, when the upstream gradient g (B, H, W, C) is given,
        grad_tex, grad_tex_abs (Bt, 6, n, n, C), grad_tex_n (Bt, 6, n, n)   d sum(g out) / d tex, terms g * weight per (pixel, tap)
        grad_uv, grad_uv_abs (B, H, W, 3), grad_uv_n (int)                  d sum(g out) / d uv
    """
    if filter_mode == "auto":
        filter_mode = "linear"
    assert filter_mode in FILTERS
    linear = filter_mode == "linear"
    tex64 = np.asarray(tex, dtype=np.float64)
    d = np.asarray(uv).astype(coords)
    Bt, six, n, n2, C = tex64.shape
    B, H, W, three = d.shape
    assert six == 6 and n == n2 and three == 3 and Bt in (1, B)
    finite, face, qs, qt, ama = _face(d, coords)
    s, t = (qs + coords(1)) * coords(0.5), (qt + coords(1)) * coords(0.5)
    bt = np.broadcast_to((np.arange(B) if Bt == B else np.zeros(B, np.int64))[:, None, None], (B, H, W))
    r = SimpleNamespace(face=face, finite=finite)

    if linear:
        x, y = s * coords(n) - coords(0.5), t * coords(n) - coords(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0).astype(np.float64), (y - y0).astype(np.float64)
        i0, j0 = np.clip(x0, -1, n - 1).astype(np.int64), np.clip(y0, -1, n - 1).astype(np.int64)
        tap_ids = ((0, 0), (1, 0), (0, 1), (1, 1))          # (dx, dy) of tap 2 dy + dx
    else:
        i0 = np.clip(np.floor(s * coords(n)), 0, n - 1).astype(np.int64)
        j0 = np.clip(np.floor(t * coords(n)), 0, n - 1).astype(np.int64)
        fx = fy = np.zeros((B, H, W))
        tap_ids = ((0, 0),)
    r.i0, r.j0 = i0, j0

    taps = []           # per tap: face, i, j (B, H, W), valid, weight before the corner rule
    drop = np.full((B, H, W), -1, np.int64)
    wc = np.zeros((B, H, W))
    for k, (dx, dy) in enumerate(tap_ids):
        i, j = i0 + dx, j0 + dy
        ox, oy = (i < 0) | (i >= n), (j < 0) | (j >= n)
        w = (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy) if linear else np.ones((B, H, W))
        both, one = ox & oy, ox ^ oy
        drop[both & finite] = k
        wc = np.where(both, w, wc)
        # fold where exactly one index is out; elsewhere feed a harmless texel and keep the tap's own
        fi = np.where(one, i, np.where(ox, -1, np.clip(i, 0, n - 1)))
        fj = np.where(one, j, np.clip(j, 0, n - 1))
        f2, i2, j2 = _fold(face, fi, fj, n)
        tf = np.where(one, f2, face)
        ti = np.where(one, i2, np.clip(i, 0, n - 1))
        tj = np.where(one, j2, np.clip(j, 0, n - 1))
        taps.append([tf, ti, tj, finite & ~both, w])
    assert not np.any(np.sum([~v & finite for _, _, _, v, _ in taps], axis=0) > 1)         # at most one tap is dropped
    r.drop = drop
    r.inside = finite & (i0 >= 0) & (j0 >= 0) & ((i0 + 1 < n) & (j0 + 1 < n) if linear else True)
    has_drop = drop >= 0
    for tap in taps:                                        # w'_k = w_k + w_c / 3; 0 for a tap without a texel
        tap[4] = np.where(tap[3], np.where(has_drop, tap[4] + wc / 3.0, tap[4]), 0.0)
    tv = [np.where(v[..., None], tex64[bt, tf, tj, ti], 0.0) for tf, ti, tj, v, _ in taps]

    if linear:
        t00, t10, t01, t11 = tv
        top = t00 + (t10 - t00) * fx[..., None]
        bot = t01 + (t11 - t01) * fx[..., None]
        plain = top + (bot - top) * fy[..., None]
        summed = sum(tap[4][..., None] * v for tap, v in zip(taps, tv))
        out = np.where(has_drop[..., None], summed, plain)
    else:
        out = tv[0]
    r.out = np.where(finite[..., None], out, 0.0)
    r.out_abs = sum(tap[4][..., None] * np.abs(v) for tap, v in zip(taps, tv))
    if g is None:
        return r

    g64 = np.asarray(g, dtype=np.float64)
    at, terms = [], []
    for tf, ti, tj, valid, w in taps:
        at.append(((bt[valid] * 6 + tf[valid]) * n + tj[valid]) * n + ti[valid])
        terms.append((g64 * w[..., None])[valid])
    gt, gt_abs, gt_n = _scatter(np.concatenate(at), np.concatenate(terms), (Bt * 6, n, n, C))
    r.grad_tex, r.grad_tex_abs, r.grad_tex_n = gt.reshape(tex64.shape), gt_abs.reshape(tex64.shape), gt_n.reshape(Bt, 6, n, n)

    r.grad_uv = np.zeros((B, H, W, 3))
    r.grad_uv_abs = np.zeros((B, H, W, 3))
    r.grad_uv_n = 4 * C
    if linear:
        # the missing texel is the mean of the other three: the lookup is bilinear in (fx, fy) in every case
        mean = sum(tv) / 3.0
        mean_abs = sum(np.abs(v) for v in tv) / 3.0
        full = [np.where((drop == k)[..., None], mean, v) for k, v in enumerate(tv)]
        fabs = [np.where((drop == k)[..., None], mean_abs, np.abs(v)) for k, v in enumerate(tv)]
        t00, t10, t01, t11 = full
        a00, a10, a01, a11 = fabs
        ofx, ofy, fxe, fye = (1.0 - fx)[..., None], (1.0 - fy)[..., None], fx[..., None], fy[..., None]
        gs = n * (g64 * ((t10 - t00) * ofy + (t11 - t01) * fye)).sum(-1)
        gt_ = n * (g64 * ((t01 - t00) * ofx + (t11 - t10) * fxe)).sum(-1)
        As = n * (np.abs(g64) * ((a10 + a00) * ofy + (a11 + a01) * fye)).sum(-1)
        At = n * (np.abs(g64) * ((a01 + a00) * ofx + (a11 + a10) * fxe)).sum(-1)
        am, q_s, q_t = ama.astype(np.float64), qs.astype(np.float64), qt.astype(np.float64)
        gsc, gtc = 0.5 * gs / am, 0.5 * gt_ / am
        gma = -(gsc * q_s + gtc * q_t)
        asc, atc = 0.5 * As / am, 0.5 * At / am
        ama_ = asc * np.abs(q_s) + atc * np.abs(q_t)
        r.grad_uv = np.stack(_to_dir(face, gsc, gtc, gma), axis=-1)
        r.grad_uv_abs = np.abs(np.stack(_to_dir(face, asc, atc, ama_), axis=-1))
        r.grad_uv[~finite] = 0.0
        r.grad_uv_abs[~finite] = 0.0
    return r
