"""
The texture lookup of largesteps.render.texture, stated in vectorised numpy (the yardstick of tests/test_texture_cpu.py and
tests/test_texture_gpu.py; nvdiffrast's semantics without mipmaps, written from the contract and not from the kernel).

tex (Bt, Ht, Wt, C) with Bt in {1, B}, uv (B, H, W, 2). Texel (i, j) has its centre at ((i + 0.5) / Wt, (j + 0.5) / Ht).

    linear    x = u Wt - 0.5, y = v Ht - 0.5 (one multiply, one subtract, in the coordinate type), i0 = floor(x), fx = x - i0, likewise
              j0, fy; taps (i0, j0) (i0 + 1, j0) (i0, j0 + 1) (i0 + 1, j0 + 1);
              out = top + (bot - top) fy,  top = t00 + (t10 - t00) fx,  bot = t01 + (t11 - t01) fx
    nearest   the texel (floor(u Wt), floor(v Ht))
    boundary  per tap index: wrap = modulo the size, clamp = clamped to [0, size - 1], zero = a tap outside reads 0 and gets no gradient
    floor(x) becomes an integer by a saturating int32 conversion (the last float below 2^31 is 2^31 - 128); a non-finite x or y
    gives output 0 and no gradient.

Coordinates and fractions are computed in `coords` (np.float32: exactly the numbers the device uses; np.float64: for finite
differences, which fp32 fractions would drown); everything after them in fp64. Every returned sum comes with the sum of the absolute
values of the terms that were added and their number, for the error bounds of the device tests.
"""
from types import SimpleNamespace

import numpy as np

FILTERS = ("nearest", "linear")
BOUNDARIES = ("wrap", "clamp", "zero")


def _axis(c, n, linear, coords):
    """coordinate c (array of `coords`) along an axis of n texels -> (finite, i0 int64, f fp64)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = c * coords(n)
        if linear:
            x = x - coords(0.5)
        finite = np.isfinite(x)
        x0 = np.floor(x)
        f = np.where(finite, x - x0, 0).astype(np.float64)
    i0 = np.clip(np.where(finite, x0, 0), -2.0 ** 31, 2.0 ** 31 - 128).astype(np.int64)
    return finite, i0, f


def _fold(i, n, boundary):
    """tap index -> (index in [0, n), valid)"""
    if boundary == "wrap":
        return np.mod(i, n), np.ones(i.shape, bool)
    if boundary == "clamp":
        return np.clip(i, 0, n - 1), np.ones(i.shape, bool)
    if boundary == "zero":
        return np.clip(i, 0, n - 1), (i >= 0) & (i < n)
    raise ValueError(boundary)


def _scatter(at, term, shape):
    """(sum of term (n, C), sum of |term|, number of terms) per flat texel index `at` (n) of a texture of `shape` (Bt, Ht, Wt, C), the
    terms of one texel added in the order given: np.bincount adds in input order from 0.0, the very additions of np.add.at into zeros,
    at a fraction of the cost (a 4096 x 4096 texture takes well under a second)"""
    size, C = shape[0] * shape[1] * shape[2], shape[3]
    grad, grad_abs = np.empty((size, C)), np.empty((size, C))
    for c in range(C):
        grad[:, c] = np.bincount(at, weights=term[:, c], minlength=size)
        grad_abs[:, c] = np.bincount(at, weights=np.abs(term[:, c]), minlength=size)
    return grad.reshape(shape), grad_abs.reshape(shape), np.bincount(at, minlength=size).astype(np.int64).reshape(shape[:3])


def texture(tex, uv, g=None, filter_mode="linear", boundary_mode="wrap", coords=np.float32):
    """
    Returns a namespace with
        out, out_abs (B, H, W, C)                       the lookup and the sum of |weight * texel| over its taps
        i0, j0 (B, H, W) int64, finite (B, H, W) bool   the base tap (before the boundary rule)
    and, when the upstream gradient g (B, H, W, C) is given,
        grad_tex, grad_tex_abs (Bt, Ht, Wt, C), grad_tex_n (Bt, Ht, Wt)   d sum(g out) / d tex, terms g * weight per (pixel, tap)
        grad_uv, grad_uv_abs (B, H, W, 2), grad_uv_n (int)               d sum(g out) / d uv, terms +-size * g * texel * weight
    """
    if filter_mode == "auto":
        filter_mode = "linear"
    assert filter_mode in FILTERS and boundary_mode in BOUNDARIES
    linear = filter_mode == "linear"
    tex64 = np.asarray(tex, dtype=np.float64)
    uvc = np.asarray(uv).astype(coords)
    Bt, Ht, Wt, C = tex64.shape
    B, H, W, _ = uvc.shape
    assert Bt in (1, B)
    finx, i0, fx = _axis(uvc[..., 0], Wt, linear, coords)
    finy, j0, fy = _axis(uvc[..., 1], Ht, linear, coords)
    finite = finx & finy
    bt = np.broadcast_to((np.arange(B) if Bt == B else np.zeros(B, np.int64))[:, None, None], (B, H, W))
    r = SimpleNamespace(i0=i0, j0=j0, finite=finite)

    taps = []           # (dx, dy, i, j, valid, t (B, H, W, C) with 0 where invalid)
    for dy in ((0, 1) if linear else (0,)):
        for dx in ((0, 1) if linear else (0,)):
            i, vx = _fold(i0 + dx, Wt, boundary_mode)
            j, vy = _fold(j0 + dy, Ht, boundary_mode)
            valid = vx & vy & finite
            taps.append((dx, dy, i, j, valid, np.where(valid[..., None], tex64[bt, j, i], 0.0)))

    def weight(dx, dy):
        return (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy) if linear else np.ones_like(fx)

    if linear:
        t00, t10, t01, t11 = (t[5] for t in taps)
        top = t00 + (t10 - t00) * fx[..., None]
        bot = t01 + (t11 - t01) * fx[..., None]
        out = top + (bot - top) * fy[..., None]
    else:
        out = taps[0][5]
    r.out = np.where(finite[..., None], out, 0.0)
    r.out_abs = sum(np.abs(t[5]) * weight(t[0], t[1])[..., None] for t in taps)
    if g is None:
        return r

    g64 = np.asarray(g, dtype=np.float64)
    at, terms = [], []
    for dx, dy, i, j, valid, _ in taps:
        at.append((bt[valid] * Ht + j[valid]) * Wt + i[valid])
        terms.append((g64 * weight(dx, dy)[..., None])[valid])
    r.grad_tex, r.grad_tex_abs, r.grad_tex_n = _scatter(np.concatenate(at), np.concatenate(terms), tex64.shape)

    r.grad_uv = np.zeros((B, H, W, 2))
    r.grad_uv_abs = np.zeros((B, H, W, 2))
    r.grad_uv_n = 4 * C
    if linear:
        ofx, ofy = (1.0 - fx)[..., None], (1.0 - fy)[..., None]
        fxe, fye = fx[..., None], fy[..., None]
        a00, a10, a01, a11 = (np.abs(t) for t in (t00, t10, t01, t11))
        r.grad_uv[..., 0] = Wt * (g64 * ((t10 - t00) * ofy + (t11 - t01) * fye)).sum(-1)
        r.grad_uv[..., 1] = Ht * (g64 * ((t01 - t00) * ofx + (t11 - t10) * fxe)).sum(-1)
        r.grad_uv_abs[..., 0] = Wt * (np.abs(g64) * ((a10 + a00) * ofy + (a11 + a01) * fye)).sum(-1)
        r.grad_uv_abs[..., 1] = Ht * (np.abs(g64) * ((a01 + a00) * ofx + (a11 + a10) * fxe)).sum(-1)
        r.grad_uv[~finite] = 0.0
        r.grad_uv_abs[~finite] = 0.0
    return r
