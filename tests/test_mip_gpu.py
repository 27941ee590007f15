"""
The mipmapped `texture`, `texture_construct_mip`, `pixel_differentials` and `interpolate(diff_attrs=...)` of largesteps.render on the
device against tests/mip_statement.py (the fp64 numpy specification) with derived bounds, against a plain-torch pyramid (bit for bit),
against themselves (two runs, cached and fresh order, captured and eager) and through the whole chain
rasterize -> interpolate(diff) -> texture(mip) -> antialias against central differences of the composed statements.

Bounds (U = 2^-24; the statement shares the device's fp32 coordinates, fractions and pyramid and continues in fp64):
  lod        an fp32 lod is within dlod = 16 U (1 + |lod|) of the statement's: m is a sum of non-negative terms plus a square root no
             larger than them (a few U relative), half a log2 of that is under 6 U absolute, log2f and the bias addition add about
             U |lod| each.
  forward    |err| <= 16 U max|tex| + |d out / d lod| dlod.
  gradients  an entry that sums n terms of magnitude sum S: |err| <= (n + 16) U S + |d entry / d lod| dlod (the statement reports n, S
             and the last term).
Level selection is a floor: the statement flags the pixels whose lod (lod + 1/2 in nearest mode) lies within 64 U (1 + |lod|) of an
integer; they are left out of the gradient comparison (their upstream gradient is zeroed) and, in nearest mode, of the forward one. At
most 2 % of a case's pixels may be flagged (tests/test_mip_cpu.py checks the cases without a device).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mip_statement as ms  # noqa: E402
import render_statement as rs  # noqa: E402
import texture_statement as ts  # noqa: E402
from render_scenes import clip, look_at, scene  # noqa: E402
from texture_cases import scaled_da as _scaled_da  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = 2.0 ** -24
CASES = ["b1_8x8_c3", "b2_shared_4x2_c4", "b2_own_16x16_c1_max2", "one_texel", "c7", "bias_only", "constant_uv", "nonfinite", "interpolated"]
COMBOS = [(m, b) for m in ms.MODES for b in ts.BOUNDARIES]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def oblique_quad():
    """(pos (1, 4, 4), tri (2, 3), uv attribute (4, 2), H, W): a two-triangle quad seen obliquely under perspective"""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    attr = np.array([[0.1, 0.05], [1.7, 0.2], [1.5, 1.9], [-0.2, 1.6]], np.float32)
    return clip(v, [look_at((1.8, 1.1, -1.9))], ar=24 / 20), np.array([[0, 1, 2], [0, 2, 3]]), attr, 20, 24


def case(name, device_chain=False):
    """(tex, uv, uv_da or None, bias or None, max_mip_level) fp32 arrays. device_chain: 'interpolated' takes uv and uv_da from the device's
    own rasterize -> interpolate(diff_attrs='all') instead of the statements'."""
    rng = np.random.default_rng(sum(map(ord, name)))

    def make(B, H, W, Bt, Ht, Wt, C, lo=-1.0, hi=2.0, max_level=None):
        Lmax = ms.last_level(Ht, Wt, max_level)
        tex = rng.standard_normal((Bt, Ht, Wt, C)).astype(np.float32)
        uv = rng.uniform(lo, hi, (B, H, W, 2)).astype(np.float32)
        da = _scaled_da(rng, (B, H, W), Ht, Wt, -0.8, Lmax + 0.8)          # with the bias: lod spread over [-1, Lmax + 1], both clamps hit
        bias = rng.uniform(-0.2, 0.2, (B, H, W)).astype(np.float32)
        return tex, uv, da, bias, max_level

    if name == "b1_8x8_c3":
        return make(1, 9, 9, 1, 8, 8, 3)
    if name == "b2_shared_4x2_c4":              # 4 x 2 -> 2 x 1 -> 1 x 1: a 1-wide level; the float4 path
        return make(2, 6, 5, 1, 2, 4, 4)
    if name == "b2_own_16x16_c1_max2":
        return make(2, 7, 6, 2, 16, 16, 1, max_level=2)
    if name == "one_texel":                     # Lmax = 0
        return make(2, 5, 5, 2, 1, 1, 4)
    if name == "c7":                            # two channel groups
        return make(2, 8, 8, 1, 4, 8, 7)
    if name == "bias_only":
        tex, uv, _, _, _ = make(1, 9, 9, 1, 8, 8, 3)
        return tex, uv, None, rng.uniform(-1.0, 4.0, (1, 9, 9)).astype(np.float32), None
    if name == "constant_uv":                   # 2048 pixels on one cell at lod 1.37: the wave-wide sum into two levels, and the fold
        tex, uv, _, _, _ = make(2, 32, 32, 1, 4, 8, 3, 0.0, 1.0)
        uv[...] = np.float32([0.62, 0.4])
        return tex, uv, None, np.full((2, 32, 32), 1.37, np.float32), None
    if name == "nonfinite":
        tex, uv, da, bias, _ = make(1, 9, 9, 1, 8, 8, 3)
        uv[0, 1, 2, 0] = np.nan
        da[0, 3, 4, 2] = np.inf
        bias[0, 5, 6] = np.nan
        uv[0, 7, 7, 1] = -np.inf
        return tex, uv, da, bias, None
    if name == "interpolated":
        pos, tri, attr, H, W = oblique_quad()
        tex = rng.standard_normal((1, 16, 16, 3)).astype(np.float32)
        if device_chain:
            import largesteps.render as dr
            rast, rast_db = dr.rasterize(None, dev(pos), dev(tri), (H, W))
            uv, da = dr.interpolate(dev(attr), rast, dev(tri), rast_db=rast_db, diff_attrs='all')
            return tex, uv.cpu().numpy(), da.cpu().numpy(), None, None
        rast = rs.rasterize(pos, tri, H, W)
        db, _ = ms.pixel_differentials(rast, pos, tri)
        return tex, rs.interpolate(attr, rast, tri), ms.attr_da(attr, rast, tri, db)[0].astype(np.float32), None, None
    raise KeyError(name)


def _run(tex, uv, da, bias, g, mode, boundary, max_level, mip=False):
    import largesteps.render as dr
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
    d = None if da is None else dev(da).requires_grad_(True)
    b = None if bias is None else dev(bias).requires_grad_(True)
    m = dr.texture_construct_mip(t, max_mip_level=max_level) if mip else None
    out = dr.texture(t, c, d, b, mip=m, filter_mode=mode, boundary_mode=boundary, max_mip_level=max_level)
    (out * dev(g)).sum().backward()
    z = lambda x: None if x is None else x.grad.cpu().numpy()  # noqa: E731
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), c.grad.cpu().numpy(), z(d), z(b)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode,boundary", COMBOS)
def test_native_matches_statement(mode, boundary, name):
    tex, uv, da, bias, max_level = case(name, device_chain=True)
    C = tex.shape[3]
    g = np.random.default_rng(1).standard_normal(uv.shape[:3] + (C,)).astype(np.float32)
    flag = ms.texture(tex, uv, da, bias, None, mode, boundary, max_level).flag
    assert flag.mean() <= 0.02, (name, flag.mean())
    if name in ("constant_uv", "bias_only"):
        assert not flag.any()
    g = g * ~flag[..., None]
    out, gt, gc, gd, gb = _run(tex, uv, da, bias, g, mode, boundary, max_level, mip=(name == "b1_8x8_c3"))
    r = ms.texture(tex, uv, da, bias, g, mode, boundary, max_level)
    linear = mode == "linear-mipmap-linear"
    keep = np.ones_like(flag) if linear else ~flag
    e_out = np.abs(out - r.out)
    b_out = 16 * U * np.abs(tex).max() + np.abs(r.dout_dlod) * r.dlod[..., None]
    e_t, b_t = np.abs(gt - r.grad_tex), (r.grad_tex_n[..., None] + 16) * U * r.grad_tex_abs + r.grad_tex_lod
    e_c, b_c = np.abs(gc - r.grad_uv), (r.grad_uv_n + 16) * U * r.grad_uv_abs + r.grad_uv_lod
    rel = lambda e, b: float((e / np.maximum(b, 1e-300)).max())  # noqa: E731
    print(f"{name} {mode} {boundary}: flagged {int(flag.sum())}; forward err/bound {rel(e_out[keep], b_out[keep]):.3f}; grad_tex {rel(e_t, b_t):.3f} "
          f"(max terms {r.grad_tex_n.max()}); grad_uv {rel(e_c, b_c):.3f}")
    for a in (out, gt, gc, gd, gb):
        assert a is None or np.all(np.isfinite(a))
    assert np.all(e_out[keep] <= b_out[keep])
    assert np.all(e_t <= b_t)
    assert np.all(e_c <= b_c)
    if bias is not None:
        e_b, b_b = np.abs(gb - r.grad_bias), (r.grad_bias_n + 16) * U * r.grad_bias_abs
        print(f"    grad_bias {rel(e_b, b_b):.3f}")
        assert np.all(e_b <= b_b)
        assert linear or not gb.any()
    if da is not None:
        e_d, b_d = np.abs(gd - r.grad_uv_da), (r.grad_uv_da_n + 16) * U * r.grad_uv_da_abs
        print(f"    grad_uv_da {rel(e_d, b_d):.3f}")
        assert np.all(e_d <= b_d)
        assert linear or not gd.any()
    if name == "constant_uv":
        assert r.grad_tex_n.max() >= 2048 and r.two.all() == linear
    if name == "nonfinite":
        bad = ~r.finite
        assert bad.sum() == 4 and not out[bad].any() and not gc[bad].any() and not gd[bad].any() and not gb[bad].any()
    if linear and name in ("b1_8x8_c3", "c7"):
        lc = np.clip(r.lod, 0, r.Lmax)
        assert (r.lod < 0).any() and (r.lod > r.Lmax).any() and r.two.any()
        assert not gb[(lc != r.lod)].any()                 # no slope where lod was clamped


def _torch_pyramid(t, Lmax):
    levels = [t]
    for _ in range(Lmax):
        H, W = t.shape[1], t.shape[2]
        if H > 1 and W > 1:
            t = ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])) * 0.25
        elif W > 1:
            t = (t[:, :, 0::2] + t[:, :, 1::2]) * 0.5
        else:
            t = (t[:, 0::2] + t[:, 1::2]) * 0.5
        levels.append(t)
    return levels


def _texel_centres(n):
    """fp32 coordinates u_k, k < n, whose texel-space coordinate u_k n - 0.5 is exactly k in the device's fp32 arithmetic (fx = 0: the
    lookup returns the texel's own bits): (k + 0.5) / n correctly rounded, or one of its neighbours. (torch divides by a scalar on
    the device by multiplying with its reciprocal, which misses for sizes that are no power of two.) Such a number need not exist for
    every k of every size; it does for the sizes used here. The check below multiplies and subtracts in two rounded steps, as the
    device does because the library is built with -ffp-contract=off (csrc/Makefile); a contracted x n - 0.5 would be one fma and
    this check would no longer describe it."""
    k = np.arange(n, dtype=np.float32)
    u = (k + np.float32(0.5)) / np.float32(n)
    cands = np.stack([u] + [np.nextafter(u, np.float32(d)) for d in (np.inf, -np.inf)])
    exact = cands * np.float32(n) - np.float32(0.5) == k
    assert cands.dtype == np.float32 and exact.any(0).all(), n
    return dev(cands[exact.argmax(0), np.arange(n)])


@pytest.mark.parametrize("shape,max_level", [((2, 8, 8, 3), None), ((1, 2, 4, 4), None), ((1, 16, 16, 1), 2), ((1, 1, 1, 2), None), ((1, 32, 2, 5), None),
                                             ((1, 64, 512, 3), None), ((1, 40, 72, 3), 3)])
def test_pyramid_levels_are_the_plain_torch_means_bit_for_bit(shape, max_level):
    import largesteps.render as dr
    tex = dev(np.random.default_rng(4).standard_normal(shape).astype(np.float32))
    mip = dr.texture_construct_mip(tex, max_mip_level=max_level)
    want = _torch_pyramid(tex, ms.last_level(shape[1], shape[2], max_level))
    assert mip.Lmax == len(want) - 1
    for l, level in enumerate(want):
        Hl, Wl = level.shape[1], level.shape[2]
        vv, uu = torch.meshgrid(_texel_centres(Hl), _texel_centres(Wl), indexing="ij")
        uv = torch.stack([uu, vv], -1)[None].expand(shape[0], -1, -1, -1).contiguous()
        bias = torch.full((shape[0], Hl, Wl), float(l), device=DEV)
        for mode in ms.MODES:
            got = dr.texture(tex, uv, mip_level_bias=bias, mip=mip, filter_mode=mode, boundary_mode="clamp")
            assert torch.equal(got, level), (l, mode)
        assert np.array_equal(level.cpu().numpy(), ms.pyramid(tex.cpu().numpy(), max_level)[l])


def _differentials_case(name):
    if name == "oblique_quad":
        pos, tri, attr, H, W = oblique_quad()
        return pos, tri, attr, H, W
    pos, tri, H, W = scene(name)
    rng = np.random.default_rng(3)
    return pos, tri, rng.standard_normal((pos.shape[1], 5)).astype(np.float32), H, W


@pytest.mark.parametrize("name", ["oblique_quad", "sphere_b3"])
def test_differentials_match_statement(name):
    import largesteps.render as dr
    pos, tri, attr, H, W = _differentials_case(name)
    tp, tf = dev(pos), dev(tri)
    rast, rast_db = dr.rasterize(None, tp, tf, (H, W))
    assert not rast_db.any()                                        # the placeholder stays zero
    db = dr.pixel_differentials(rast, tp, tf)
    rn = rast.cpu().numpy()
    want, mag = ms.pixel_differentials(rn, pos, tri)
    err = np.abs(db.cpu().numpy() - want)
    covered = rn[..., 3] > 0
    print(f"{name}: covered {covered.sum()} pixels; db worst err/bound {(err / np.maximum(16 * U * mag, 1e-300)).max():.3f}")
    assert covered.any() and np.all(err <= 16 * U * mag)
    assert not db.cpu().numpy()[~covered].any() and db.cpu().numpy()[covered].any()
    out, da = dr.interpolate(dev(attr), rast, tf, rast_db=rast_db, diff_attrs='all')
    assert not da.requires_grad and da.shape == rast.shape[:3] + (2 * attr.shape[1],)
    assert torch.equal(out, dr.interpolate(dev(attr), rast, tf)[0])
    want_da, mag_da = ms.attr_da(attr, rn, tri, want, mag)
    err = np.abs(da.cpu().numpy() - want_da)
    print(f"    attr_da worst err/bound {(err / np.maximum(16 * U * mag_da, 1e-300)).max():.3f}")
    assert np.all(err <= 16 * U * mag_da)
    assert not da.cpu().numpy()[~covered].any() and da.cpu().numpy()[covered].any()
    # a selection of channels, an explicit rast_db tensor, and the cache on the placeholder
    sel = [attr.shape[1] - 1, 0]
    part = dr.interpolate(dev(attr), rast, tf, rast_db=db.clone(), diff_attrs=sel)[1]
    assert torch.equal(part, torch.cat([da[..., 2 * c:2 * c + 2] for c in sel], -1))
    assert rast_db._largesteps_db.db is not None
    with pytest.raises(IndexError):
        dr.interpolate(dev(attr), rast, tf, rast_db=rast_db, diff_attrs=[attr.shape[1]])


def test_degenerate_faces_give_zero_differentials():
    import largesteps.render as dr
    pos = np.array([[[-1, -1, 0.5, 1], [1, -1, 0.5, 1], [1, 1, 0.5, 1], [0, 0, 0.5, 1]]], np.float32)
    tri = np.array([[0, 1, 2], [0, 3, 2]])                          # the second face has zero area (3 lies on the edge 0-2)
    rast, _ = dr.rasterize(None, dev(pos), dev(tri), (8, 8))
    fake = rast.clone()
    fake[..., 3] = torch.where(fake[..., 3] > 0, 2.0, 0.0)          # claim that every covered pixel belongs to the degenerate face
    db = dr.pixel_differentials(fake, dev(pos), dev(tri))
    assert not db.any()
    assert dr.pixel_differentials(rast, dev(pos), dev(tri)).any()


def test_attr_da_is_the_pixel_to_pixel_difference_in_an_affine_view():
    """w = 1: an attribute is affine in the pixel coordinates inside a face, so attr_da IS out[x + 1] - out[x] (and out[y + 1] - out[y])"""
    import largesteps.render as dr
    pos = np.array([[[-0.9, -0.8, 0.5, 1], [0.95, -0.6, 0.5, 1], [0.1, 0.9, 0.5, 1]]], np.float32)
    tri = np.array([[0, 1, 2]])
    attr = np.random.default_rng(5).standard_normal((3, 4)).astype(np.float32)
    H, W = 16, 20
    rast, rast_db = dr.rasterize(None, dev(pos), dev(tri), (H, W))
    out, da = dr.interpolate(dev(attr), rast, dev(tri), rast_db=rast_db, diff_attrs='all')
    rn, o, d = rast.cpu().numpy(), out.cpu().numpy().astype(np.float64), da.cpu().numpy()
    cov = rn[..., 3] > 0
    _, mag = ms.attr_da(attr, rn, tri, *ms.pixel_differentials(rn, pos, tri))
    # the two interpolated values carry their own rounding: three products of magnitude <= |a| each
    slack = 16 * U * np.abs(attr).max()
    both = cov[:, :, 1:] & cov[:, :, :-1]
    err = np.abs((o[:, :, 1:] - o[:, :, :-1]) - d[:, :, :-1, 0::2])[both]
    assert both.sum() > 20 and np.all(err <= 16 * U * mag[:, :, :-1, 0::2][both] + slack)
    both = cov[:, 1:] & cov[:, :-1]
    err = np.abs((o[:, 1:] - o[:, :-1]) - d[:, :-1, :, 1::2])[both]
    assert both.sum() > 20 and np.all(err <= 16 * U * mag[:, :-1, :, 1::2][both] + slack)


def test_the_feature_is_on():
    """fails on the parent commit: the mipmap modes raised NotImplementedError and diff_attrs raised"""
    import largesteps.render as dr
    tex = (np.indices((8, 8)).sum(0) % 2).astype(np.float32)[None, :, :, None]            # a checkerboard
    uv = np.random.default_rng(0).uniform(0, 1, (1, 9, 9, 2)).astype(np.float32)
    bias = np.full((1, 9, 9), 2.0, np.float32)
    got = dr.texture(dev(tex), dev(uv), mip_level_bias=dev(bias), filter_mode='linear-mipmap-linear')
    plain = dr.texture(dev(tex), dev(uv), filter_mode='linear')
    assert not torch.equal(got, plain)
    want = ms.texture(tex, uv, None, bias, None, 'linear-mipmap-linear', 'wrap').out
    assert np.abs(got.cpu().numpy() - want).max() <= 16 * U
    assert np.abs(want - 0.5).max() <= 1e-12                        # two levels up a checkerboard is grey
    pos, tri, attr, H, W = oblique_quad()
    rast, rast_db = dr.rasterize(None, dev(pos), dev(tri), (H, W))
    da = dr.interpolate(dev(attr), rast, dev(tri), rast_db=rast_db, diff_attrs='all')[1]
    assert (da[rast[..., 3] > 0].abs().sum(-1) > 0).all()
    with pytest.raises(ValueError):
        dr.texture(dev(tex), dev(uv), filter_mode='linear-mipmap-linear')
    with pytest.raises(ValueError, match="level 0 is 6 x 5"):
        dr.texture(dev(np.zeros((1, 6, 5, 1), np.float32)), dev(uv), mip_level_bias=dev(bias), filter_mode='linear-mipmap-nearest')
    t = dev(tex)
    mip = dr.texture_construct_mip(t)
    assert torch.equal(dr.texture(t, dev(uv), mip_level_bias=dev(bias), mip=mip, filter_mode='linear-mipmap-linear'), got)
    t.mul_(0.5)
    with pytest.raises(ValueError, match="stale"):
        dr.texture(t, dev(uv), mip_level_bias=dev(bias), mip=mip, filter_mode='linear-mipmap-linear')


def test_two_runs_and_cached_order_are_bitwise_identical():
    import largesteps.render as dr
    for name in ("b2_shared_4x2_c4", "constant_uv", "b2_own_16x16_c1_max2"):
        tex, uv, da, bias, max_level = case(name)
        g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (tex.shape[3],)).astype(np.float32)
        for mode, boundary in COMBOS:
            a = _run(tex, uv, da, bias, g, mode, boundary, max_level)
            b = _run(tex, uv, da, bias, g, mode, boundary, max_level, mip=True)
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(x, y)
            t, c, d, bb, gg = dev(tex).requires_grad_(True), dev(uv), dev(da), dev(bias), dev(g)
            kw = dict(filter_mode=mode, boundary_mode=boundary, max_mip_level=max_level)
            (dr.texture(t, c, d, bb, **kw) * gg).sum().backward()
            slot = c._largesteps_mip_order
            assert slot.order is not None
            first, t.grad = t.grad.clone(), None
            (dr.texture(t, c, d, bb, **kw) * gg).sum().backward()
            assert c._largesteps_mip_order is slot
            assert torch.equal(t.grad, first) and np.array_equal(first.cpu().numpy(), a[1])


def test_changing_uv_da_in_place_invalidates_the_cached_order():
    import largesteps.render as dr
    tex, uv, da, bias, _ = case("b1_8x8_c3")
    g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (3,)).astype(np.float32)
    t, c, d, b, gg = dev(tex).requires_grad_(True), dev(uv), dev(da), dev(bias), dev(g)
    kw = dict(filter_mode='linear-mipmap-linear')
    (dr.texture(t, c, d, b, **kw) * gg).sum().backward()
    slot = c._largesteps_mip_order
    d.mul_(1.7)
    t.grad = None
    (dr.texture(t, c, d, b, **kw) * gg).sum().backward()
    assert c._largesteps_mip_order is not slot
    assert np.array_equal(t.grad.cpu().numpy(), _run(tex, uv, d.cpu().numpy(), bias, g, 'linear-mipmap-linear', 'wrap', None)[1])


def test_a_level_of_the_pyramid_is_read_exactly_as_a_plain_texture():
    """With mip_level_bias all zero and no uv_da the level of detail is 0 and level 0 alone is read: both mip modes return the bits of
    texture(tex, uv, 'linear', boundary) -- forward, gradient to tex and gradient to uv -- with max_mip_level=0 and with the full pyramid
    (the fold then adds the zero gradients of the upper levels), and the gradient to the bias is exactly zero. uv is uniform in [-1, 2],
    so taps fall outside under every boundary mode; 2048 pixels give the 8 x 8 texture more than 64 items per texel (the wave-wide sum)
    and the 64 x 64 textures fewer."""
    import largesteps.render as dr
    rng = np.random.default_rng(11)
    uv = rng.uniform(-1.0, 2.0, (2, 32, 32, 2)).astype(np.float32)

    def bits(x):
        return x.contiguous().view(torch.int32)

    for Bt, Ht in ((1, 8), (2, 64)):
        for C in (3, 4, 5):
            tex = rng.standard_normal((Bt, Ht, Ht, C)).astype(np.float32)
            g = dev(rng.standard_normal((2, 32, 32, C)).astype(np.float32))
            for boundary in ts.BOUNDARIES:
                t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
                want = dr.texture(t, c, filter_mode='linear', boundary_mode=boundary)
                (want * g).sum().backward()
                for mode in ms.MODES:
                    for max_level in (0, None):
                        tm, cm = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
                        bias = torch.zeros((2, 32, 32), dtype=torch.float32, device=DEV).requires_grad_(True)
                        got = dr.texture(tm, cm, mip_level_bias=bias, filter_mode=mode, boundary_mode=boundary, max_mip_level=max_level)
                        (got * g).sum().backward()
                        what = (Bt, Ht, C, boundary, mode, max_level)
                        assert torch.equal(bits(got), bits(want)), ("forward",) + what
                        assert torch.equal(bits(tm.grad), bits(t.grad)), ("grad tex",) + what
                        assert torch.equal(bits(cm.grad), bits(c.grad)), ("grad uv",) + what
                        assert bias.grad is not None and torch.count_nonzero(bias.grad) == 0, ("grad bias",) + what


def _chain_device(tp, tf, ta, tt, H, W):
    import largesteps.render as dr
    rast, rast_db = dr.rasterize(None, tp, tf, (H, W))
    uv, uv_da = dr.interpolate(ta, rast, tf, rast_db=rast_db, diff_attrs='all')
    return dr.antialias(dr.texture(tt, uv, uv_da, filter_mode='linear-mipmap-linear'), rast, tp, tf)


def test_captured_chain_matches_eager():
    pos, tri, attr, H, W = oblique_quad()
    rng = np.random.default_rng(6)
    g = dev(rng.standard_normal((1, H, W, 3)).astype(np.float32))
    tp, tf = dev(pos).requires_grad_(True), dev(tri)
    ta, tt = dev(attr).requires_grad_(True), dev(rng.uniform(0, 1, (1, 16, 16, 3)).astype(np.float32)).requires_grad_(True)

    def body(p=tp, a=ta, t=tt):
        p.grad = a.grad = t.grad = None
        img = _chain_device(p, tf, a, t, H, W)
        (img * g).sum().backward()
        return img.detach(), p.grad, a.grad, t.grad

    from largesteps.capture import CapturedStep
    step = CapturedStep(body)                                      # a torch.cuda.graph capture after warm-up runs on a side stream
    for it in range(3):
        with torch.no_grad():
            tt.mul_(0.9).add_(0.02 * it)
        got = [x.clone() for x in step()]
        want = body(*(x.detach().clone().requires_grad_(True) for x in (tp, ta, tt)))
        for x, y in zip(got, want):
            assert torch.equal(x, y), it


def _chain_statement(pos, f, attr, tex, uv_da, H, W):
    """the chain by the statements, with uv_da held fixed (the device does not differentiate through it): (rast, lookup, image)"""
    rast = rs.rasterize(pos, f, H, W)
    uv = rs.interpolate(attr, rast, f)
    r = ms.texture(tex, uv, uv_da, None, None, 'linear-mipmap-linear', 'wrap', coords=np.float64)
    return rast, r, rs.antialias(r.out, rast, pos, f).astype(np.float64)


def test_chain_gradients_match_finite_differences_of_the_statements():
    """d loss / d tex and d loss / d uv-attribute of rasterize -> interpolate(diff) -> texture(mip) -> antialias against central
    differences of the composed statements in random directions, with the step and tolerances of
    test_texture_gpu.test_chain_gradients_match_finite_differences_of_the_statements. Only pixels whose level and base taps are the
    same in the three evaluations are summed (the lookup has kinks where uv crosses a texel centre line of either level)."""
    pos, f, attr, H, W = oblique_quad()
    rng = np.random.default_rng(7)
    tex = rng.uniform(0, 1, (1, 16, 16, 3)).astype(np.float32)
    g = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    eps = 2e-4
    rast0 = rs.rasterize(pos, f, H, W)
    uv_da = ms.attr_da(attr, rast0, f, ms.pixel_differentials(rast0, pos, f)[0])[0].astype(np.float32)
    _, x0, _ = _chain_statement(pos, f, attr, tex, uv_da, H, W)
    for trial in range(3):
        da_ = rng.standard_normal(attr.shape).astype(np.float32)
        dt = rng.standard_normal(tex.shape).astype(np.float32)
        _, xp, ip = _chain_statement(pos, f, attr + np.float32(eps) * da_, tex, uv_da, H, W)
        _, xm, im = _chain_statement(pos, f, attr - np.float32(eps) * da_, tex, uv_da, H, W)
        keep = (rast0[..., 3] > 0) & (xp.l0 == x0.l0) & (xm.l0 == x0.l0) & (xp.base == x0.base).all(-1) & (xm.base == x0.base).all(-1)
        assert keep.sum() > 0.5 * (rast0[..., 3] > 0).sum()
        w = g * keep[..., None]
        fd_attr = float(((ip - im) * w).sum() / (2 * eps))
        tp_, tm_ = (_chain_statement(pos, f, attr, tex + s * np.float32(eps) * dt, uv_da, H, W)[2] for s in (1, -1))
        fd_tex = float(((tp_ - tm_) * w).sum() / (2 * eps))
        ta, tt = dev(attr).requires_grad_(True), dev(tex).requires_grad_(True)
        (_chain_device(dev(pos), dev(f), ta, tt, H, W) * dev(w.astype(np.float32))).sum().backward()
        an_attr = float((ta.grad.double() * dev(da_).double()).sum())
        an_tex = float((tt.grad.double() * dev(dt).double()).sum())
        print(f"trial {trial}: kept {keep.sum()} pixels; attr fd {fd_attr:.6f} an {an_attr:.6f}; tex fd {fd_tex:.6f} an {an_tex:.6f}")
        assert abs(an_attr) > 1.0 and abs(fd_attr - an_attr) <= 0.03 * abs(an_attr), ("attr", trial, fd_attr, an_attr)
        assert abs(an_tex) > 1.0 and abs(fd_tex - an_tex) <= 0.03 * abs(an_tex), ("tex", trial, fd_tex, an_tex)
