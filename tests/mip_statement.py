"""
The mipmapped texture lookup and the pixel differentials of largesteps.render, stated in vectorised numpy (the yardstick of
tests/test_mip_cpu.py and tests/test_mip_gpu.py; written from the rules of DESIGN.md section 2.7, not from the kernel). One level is
looked up by tests/texture_statement.py: the tap rules are the plain lookup's.

Pyramid     level 0 is tex; level l + 1 has max(W_l / 2, 1) x max(H_l / 2, 1) texels; building it needs each of W_l, H_l to be 1 or even
            (ValueError otherwise); the last level Lmax is 1 x 1, or max_mip_level if that comes first. A texel is the mean of its
            2 x 2 children, IN FP32 as ((c00 + c10) + (c01 + c11)) * 0.25 ((a + b) * 0.5 when one side is already 1): `pyramid` does
            these very fp32 operations, so a device pyramid can be compared bit for bit.
Level       uv_da = (du/dX, du/dY, dv/dX, dv/dY): sx = du/dX Wt, sy = du/dY Wt, tx = dv/dX Ht, ty = dv/dY Ht; A = sx^2 + tx^2,
            B = sy^2 + ty^2, Cc = sx sy + tx ty; m = (A + B) / 2 + sqrt((A - B)^2 / 4 + Cc^2); lod = log2(m) / 2 + bias (bias = 0 when
            None; m = 0: -inf); without uv_da, lod = bias. Then clamped to [0, Lmax]. All in fp64 from the fp32 inputs.
Lookup      linear-mipmap-linear: l0 = floor(lod), l1 = min(l0 + 1, Lmax), f = lod - l0, out = c0 + (c1 - c0) f; when f == 0 or
            l0 == Lmax only l0 is read. linear-mipmap-nearest: the level min(floor(lod + 1/2), Lmax). A pixel with a non-finite uv
            (or level-0 texel coordinate), uv_da or bias outputs 0 and gives no gradient.
Gradients   to tex through every level (the transpose of the pyramid: every child gains 0.25 or 0.5 of its parent's gradient), to uv
            from both levels, d loss / d lod = sum_c g_c (c1_c - c0_c) where two levels were read (else 0), which is the gradient of the
            bias and, through the formula above, of uv_da (where the square root is 0: d m / d A = d m / d B = 1/2, d m / d Cc = 0).

Every sum is returned with the sum of the magnitudes of its terms and their number, and with the size of its own derivative by lod
times dlod = 16 u (1 + |lod|), the error an fp32 lod may carry: the bounds of the device tests. `flag` marks the pixels whose level
choice an fp32 lod may make differently: lod (lod + 1/2 in nearest mode) within 64 u (1 + |lod|) of an integer in [0, Lmax].
"""
from types import SimpleNamespace

import numpy as np

import texture_statement as ts

U = 2.0 ** -24
MODES = ("linear-mipmap-linear", "linear-mipmap-nearest")
F32 = np.float32


def last_level(Ht, Wt, max_mip_level=None):
    h, w, level = int(Ht), int(Wt), 0
    while (h > 1 or w > 1) and (max_mip_level is None or level < max_mip_level):
        if (h > 1 and h % 2) or (w > 1 and w % 2):
            raise ValueError(f"level {level} is {h} x {w}: each side must be 1 or even")
        h, w, level = max(h // 2, 1), max(w // 2, 1), level + 1
    return level


def pyramid(tex, max_mip_level=None):
    """the levels [tex, level 1, ..., level Lmax], each (Bt, H_l, W_l, C) fp32"""
    t = np.ascontiguousarray(tex, dtype=F32)
    levels = [t]
    for _ in range(last_level(t.shape[1], t.shape[2], max_mip_level)):
        H, W = t.shape[1], t.shape[2]
        if H > 1 and W > 1:
            t = ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])) * F32(0.25)
        elif W > 1:
            t = (t[:, :, 0::2] + t[:, :, 1::2]) * F32(0.5)
        else:
            t = (t[:, 0::2] + t[:, 1::2]) * F32(0.5)
        assert t.dtype == F32
        levels.append(t)
    return levels


def _up(a, shape):
    """a coarse level's array laid over the texels (Bt, H, W, ...) of the finer level: every child sees its parent; and the weight"""
    H, W = shape[1], shape[2]
    if H > 1:
        a = np.repeat(a, 2, axis=1)
    if W > 1:
        a = np.repeat(a, 2, axis=2)
    return a, (0.25 if (H > 1 and W > 1) else 0.5)


def footprint(uv_da, Ht, Wt):
    """(m, d m / d uv_da (..., 4), a magnitude for the rounding of that derivative (..., 4)) in fp64"""
    da = np.asarray(uv_da, dtype=np.float64)
    sx, sy, tx, ty = da[..., 0] * Wt, da[..., 1] * Wt, da[..., 2] * Ht, da[..., 3] * Ht
    A, B, Cc = sx * sx + tx * tx, sy * sy + ty * ty, sx * sy + tx * ty
    R = np.sqrt(0.25 * (A - B) ** 2 + Cc * Cc)
    m = 0.5 * (A + B) + R
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = R > 0
        h = np.where(pos, 0.25 * (A - B) / R, 0.0)
        dA, dB, dC = 0.5 + h, 0.5 - h, np.where(pos, Cc / R, 0.0)
        # A - B and Cc are differences of products: their rounding error is relative to A + B and |sx sy| + |tx ty|, not to themselves
        hA = np.where(pos, 0.25 * (A + B) / R, 0.0)
        aA, aC = 0.5 + hA, np.where(pos, (np.abs(sx * sy) + np.abs(tx * ty)) / R, 0.0)
    dm = np.stack([(dA * 2 * sx + dC * sy) * Wt, (dB * 2 * sy + dC * sx) * Wt, (dA * 2 * tx + dC * ty) * Ht, (dB * 2 * ty + dC * tx) * Ht], -1)
    mag = np.stack([(aA * 2 * np.abs(sx) + aC * np.abs(sy)) * Wt, (aA * 2 * np.abs(sy) + aC * np.abs(sx)) * Wt,
                    (aA * 2 * np.abs(tx) + aC * np.abs(ty)) * Ht, (aA * 2 * np.abs(ty) + aC * np.abs(tx)) * Ht], -1)
    return m, dm, mag


def texture(tex, uv, uv_da=None, bias=None, g=None, filter_mode="linear-mipmap-linear", boundary_mode="wrap", max_mip_level=None,
            coords=np.float32):
    """
    Returns a namespace with
        out (B, H, W, C), dout_dlod (B, H, W, C) (c1 - c0 where two levels were read), lod (unclamped) and dlod (B, H, W),
        finite, two, flag (B, H, W) bool, l0 (B, H, W) int, f (B, H, W), base (B, H, W, 4) int, Lmax, levels
    and, when the upstream gradient g (B, H, W, C) is given,
        grad_tex, grad_tex_abs, grad_tex_lod (Bt, Ht, Wt, C), grad_tex_n (Bt, Ht, Wt), level_n (a (Bt, H_l, W_l) count per level)
        grad_uv, grad_uv_abs, grad_uv_lod (B, H, W, 2), grad_uv_n
        grad_bias, grad_bias_abs (B, H, W), grad_bias_n          (d loss / d lod)
        grad_uv_da, grad_uv_da_abs (B, H, W, 4), grad_uv_da_n
    `_abs`: the sum of the magnitudes of the terms, `_n` their number, `_lod`: |d entry / d lod| dlod summed over the pixels.
    """
    assert filter_mode in MODES and boundary_mode in ts.BOUNDARIES
    if uv_da is None and bias is None:
        raise ValueError("uv_da or bias is needed")
    linear = filter_mode == "linear-mipmap-linear"
    levels = pyramid(tex, max_mip_level)
    Lmax = len(levels) - 1
    Bt, Ht, Wt, C = levels[0].shape
    uvc = np.asarray(uv).astype(coords)
    B, H, W, _ = uvc.shape
    finite = ts._axis(uvc[..., 0], Wt, True, coords)[0] & ts._axis(uvc[..., 1], Ht, True, coords)[0]
    lod = np.zeros((B, H, W))
    dm = None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if uv_da is not None:
            da = np.asarray(uv_da).astype(coords).astype(np.float64)
            finite &= np.isfinite(da).all(-1)
            m, dm, dm_mag = footprint(np.where(finite[..., None], da, 0.0), Ht, Wt)
            lod = 0.5 * np.log2(m)
        if bias is not None:
            b = np.asarray(bias).astype(coords).astype(np.float64)
            finite &= np.isfinite(b)
            lod = lod + np.where(finite, b, 0.0)
    lod = np.where(finite, lod, 0.0)
    lc = np.clip(lod, 0.0, float(Lmax))
    tol = 64 * U * (1 + np.abs(lc))
    if linear:
        l0 = np.floor(lc).astype(np.int64)
        f = lc - l0
        f = np.where(l0 >= Lmax, 0.0, f)
        l0 = np.minimum(l0, Lmax)
        x = lod
    else:
        l0 = np.minimum(np.floor(lc + 0.5).astype(np.int64), Lmax)
        f = np.zeros_like(lc)
        x = lod + 0.5
    with np.errstate(invalid="ignore"):
        near = np.round(x)
        flag = finite & np.isfinite(x) & (np.abs(x - near) <= tol) & (near >= 0) & (near <= Lmax) & (Lmax > 0)
    two = finite & (f != 0)
    r = SimpleNamespace(lod=lod, dlod=16 * U * (1 + np.abs(lc)), finite=finite, two=two, flag=flag, l0=l0, f=f, Lmax=Lmax, levels=levels)

    g64 = None if g is None else np.asarray(g, dtype=np.float64)
    per_level = []              # (level, reads (B, H, W), weight (B, H, W), sign of d weight / d lod, lookup namespace)
    for l in range(Lmax + 1):
        as0, as1 = finite & (l0 == l), two & (l0 + 1 == l)
        reads = as0 | as1
        if not reads.any():
            continue
        w = np.where(as1, f, np.where(two, 1.0 - f, 1.0)) * reads
        uv_l = np.where(reads[..., None], uvc, coords(np.nan))
        look = ts.texture(levels[l], uv_l, None if g is None else g64 * w[..., None], "linear", boundary_mode, coords=coords)
        sign = np.where(as1, 1.0, np.where(two & as0, -1.0, 0.0))
        per_level.append((l, reads, w, sign, look))
    r.out = np.zeros((B, H, W, C))
    r.out_abs = np.zeros((B, H, W, C))
    r.base = np.zeros((B, H, W, 4), dtype=np.int64)      # the base tap (i0, j0) at l0 and at l0 + 1 (0 where that level is not read)
    r.dout_dlod = np.zeros((B, H, W, C))
    lod_abs = np.zeros((B, H, W, C))            # |c1| + |c0| by taps, where two levels were read
    for l, reads, w, sign, look in per_level:
        r.out += look.out * w[..., None]
        for k, at in ((0, finite & (l0 == l)), (2, two & (l0 + 1 == l))):
            r.base[..., k] = np.where(at, look.i0, r.base[..., k])
            r.base[..., k + 1] = np.where(at, look.j0, r.base[..., k + 1])
        r.out_abs += look.out_abs * w[..., None]
        r.dout_dlod += look.out * sign[..., None]
        lod_abs += look.out_abs * np.abs(sign)[..., None]
    if g is None:
        return r

    # ---- to the texture: per level, then the transpose of the pyramid, top down
    G = [np.zeros(lv.shape) for lv in levels]
    Gabs = [np.zeros(lv.shape) for lv in levels]
    Glod = [np.zeros(lv.shape) for lv in levels]
    Gn = [np.zeros(lv.shape[:3], dtype=np.int64) for lv in levels]
    r.grad_uv = np.zeros((B, H, W, 2))
    r.grad_uv_abs = np.zeros((B, H, W, 2))
    r.grad_uv_lod = np.zeros((B, H, W, 2))
    r.grad_uv_n = 8 * C + 4
    slope_uv = np.zeros((B, H, W, 2))
    for l, reads, w, sign, look in per_level:
        G[l], Gabs[l], Gn[l] = look.grad_tex, look.grad_tex_abs, look.grad_tex_n
        r.grad_uv += look.grad_uv
        r.grad_uv_abs += look.grad_uv_abs
        with np.errstate(divide="ignore", invalid="ignore"):
            slope_uv += np.where(sign[..., None] != 0, look.grad_uv * (sign / np.where(w != 0, w, 1.0))[..., None], 0.0)
        # d term / d lod = +- g wx wy: the level's gradient of |g| dlod over the pixels that blend
        if np.any(sign != 0):
            uv_s = np.where((sign != 0)[..., None], uvc, coords(np.nan))
            Glod[l] = ts.texture(levels[l], uv_s, np.abs(g64) * r.dlod[..., None], "linear", boundary_mode, coords=coords).grad_tex_abs
    r.grad_uv_lod = np.abs(slope_uv) * r.dlod[..., None]
    r.level_n = [n.copy() for n in Gn]          # the items of every texel of every level, before the levels are folded into level 0
    for l in range(Lmax - 1, -1, -1):
        shape = levels[l].shape
        up, coef = _up(G[l + 1], shape)
        G[l] = G[l] + coef * up
        Gabs[l] = Gabs[l] + coef * _up(Gabs[l + 1], shape)[0]
        Glod[l] = Glod[l] + coef * _up(Glod[l + 1], shape)[0]
        # the parent's sum arrives with its own (n + 16) u |.| error; one multiply and one add follow
        Gn[l] = Gn[l] + _up(Gn[l + 1], shape)[0] + 2
    r.grad_tex, r.grad_tex_abs, r.grad_tex_lod, r.grad_tex_n = G[0], Gabs[0], Glod[0], Gn[0]
    r.level_grads = G

    # ---- to the level of detail
    r.grad_bias = np.where(two, (g64 * r.dout_dlod).sum(-1), 0.0)
    r.grad_bias_abs = np.where(two, (np.abs(g64) * lod_abs).sum(-1), 0.0)
    r.grad_bias_n = 10 * C
    r.grad_uv_da = np.zeros((B, H, W, 4))
    r.grad_uv_da_abs = np.zeros((B, H, W, 4))
    r.grad_uv_da_n = 10 * C + 16
    if uv_da is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(two, 1.0 / (2.0 * np.log(2.0) * np.where(two, m, 1.0)), 0.0)
        r.grad_uv_da = (r.grad_bias * k)[..., None] * dm
        r.grad_uv_da_abs = (r.grad_bias_abs * k)[..., None] * dm_mag
    return r


# ---- pixel differentials ----------------------------------------------------------------------------------------------------------------
def pixel_differentials(rast, pos, tri):
    """(db (B, H, W, 4) fp64 = (du/dX, du/dY, dv/dX, dv/dY) per pixel step, mag (B, H, W, 4): the sum of the magnitudes of the terms)"""
    rast = np.asarray(rast)
    pos = np.asarray(pos, dtype=F32).astype(np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    B, H, W, _ = rast.shape
    db, mag = np.zeros((B, H, W, 4)), np.zeros((B, H, W, 4))
    Yn, Xn = np.meshgrid((2.0 * np.arange(H) + 1.0) / H - 1.0, (2.0 * np.arange(W) + 1.0) / W - 1.0, indexing="ij")
    for b in range(B):
        ids = rast[b, :, :, 3].astype(np.int64)
        msk = (ids >= 1) & (ids <= tri.shape[0])
        if not msk.any():
            continue
        p = pos[b][tri[ids[msk] - 1]][:, :, [0, 1, 3]]             # (n, 3 corners, (x, y, w))
        a = np.stack([np.cross(p[:, 1], p[:, 2]), np.cross(p[:, 2], p[:, 0]), np.cross(p[:, 0], p[:, 1])], 1)     # rows of the adjugate
        D = (p[:, 0] * a[:, 0]).sum(-1)
        e = a[:, :, 0] * Xn[msk][:, None] + a[:, :, 1] * Yn[msk][:, None] + a[:, :, 2]
        s = e.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = e[:, 0] / s, e[:, 1] / s
            sA, sB = a[:, :, 0].sum(1), a[:, :, 1].sum(1)
            mA, mB = np.abs(a[:, :, 0]).sum(1), np.abs(a[:, :, 1]).sum(1)
            d = np.stack([(a[:, 0, 0] - u * sA) / s * (2.0 / W), (a[:, 0, 1] - u * sB) / s * (2.0 / H),
                          (a[:, 1, 0] - v * sA) / s * (2.0 / W), (a[:, 1, 1] - v * sB) / s * (2.0 / H)], -1)
            g = np.stack([(np.abs(a[:, 0, 0]) + np.abs(u) * mA) / np.abs(s) * (2.0 / W), (np.abs(a[:, 0, 1]) + np.abs(u) * mB) / np.abs(s) * (2.0 / H),
                          (np.abs(a[:, 1, 0]) + np.abs(v) * mA) / np.abs(s) * (2.0 / W), (np.abs(a[:, 1, 1]) + np.abs(v) * mB) / np.abs(s) * (2.0 / H)], -1)
        ok = (s != 0) & (D != 0) & np.isfinite(s) & np.isfinite(D) & np.isfinite(d).all(-1)
        db[b][msk] = np.where(ok[:, None], d, 0.0)
        mag[b][msk] = np.where(ok[:, None], g, 0.0)
    return db, mag


def attr_da(attr, rast, tri, db, db_mag=None):
    """(attr_da (B, H, W, 2 C) fp64 = [da_c/dX, da_c/dY] per channel, mag): da/dX = du/dX (a0 - a2) + dv/dX (a1 - a2)"""
    attr = np.asarray(attr, dtype=F32).astype(np.float64)
    if attr.ndim == 2:
        attr = attr[None]
    tri = np.asarray(tri, dtype=np.int64)
    rast = np.asarray(rast)
    B, H, W, _ = rast.shape
    C = attr.shape[2]
    db_mag = np.abs(db) if db_mag is None else db_mag
    out, mag = np.zeros((B, H, W, 2 * C)), np.zeros((B, H, W, 2 * C))
    for b in range(B):
        a = attr[0 if attr.shape[0] == 1 else b]
        ids = rast[b, :, :, 3].astype(np.int64)
        msk = (ids >= 1) & (ids <= tri.shape[0])
        t = tri[ids[msk] - 1]
        a0, a1, a2 = a[t[:, 0]], a[t[:, 1]], a[t[:, 2]]
        d, dmg = db[b][msk], db_mag[b][msk]
        o, g = np.zeros((msk.sum(), 2 * C)), np.zeros((msk.sum(), 2 * C))
        for k in (0, 1):                                            # X, Y
            o[:, k::2] = d[:, k, None] * (a0 - a2) + d[:, 2 + k, None] * (a1 - a2)
            g[:, k::2] = dmg[:, k, None] * (np.abs(a0) + np.abs(a2)) + dmg[:, 2 + k, None] * (np.abs(a1) + np.abs(a2))
        out[b][msk], mag[b][msk] = o, g
    return out, mag
