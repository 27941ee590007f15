"""
largesteps.render.texture on the device against tests/texture_statement.py (the numpy specification) with derived bounds, against the
plain-torch lookup it replaced (bit for bit), against itself (two runs, cached and fresh pixel order, captured and eager), and through
the whole chain rasterize -> interpolate -> texture -> antialias against central differences of the statements.

Bounds (u = 2^-24, the unit roundoff of fp32; the statement shares the device's fp32 fractions and continues in fp64):
  forward    |err| <= 16 u max|tex|: (t10 - t00), * fx, + t00 for top and for bot, then (bot - top), * fy, + top: nine roundings, each
             of a quantity of at most 2 max|tex|.
  gradients  an entry that sums n terms: |err| <= (n + 16) u S, S the sum of the terms' absolute values: n - 1 additions and at most
             three roundings inside a term (1 - f, the product of the two weights, times g; for uv: the texel difference, 1 - f, the
             product, the sum of the two products, times g, times the size).
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

import render_statement as rs  # noqa: E402
import texture_statement as ts  # noqa: E402
from render_scenes import scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = 2.0 ** -24
MODES = [(f, b) for f in ts.FILTERS for b in ts.BOUNDARIES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _interpolated_uv():
    """uv (1, 24, 32, 2) from a real interpolate of a per-vertex uv attribute over the sphere scene (background pixels: uv = 0)"""
    import largesteps.render as dr
    pos, f, H, W = scene("sphere")
    attr = (0.5 + 0.9 * pos[0, :, :2] / np.abs(pos[0, :, :2]).max()).astype(np.float32)
    rast = dr.rasterize(None, dev(pos), dev(f), (H, W))[0]
    return dr.interpolate(dev(attr), rast, dev(f))[0].cpu().numpy()


def _case(name):
    """(tex, uv) fp32 arrays"""
    rng = np.random.default_rng(sum(map(ord, name)))

    def make(B, H, W, Bt, Ht, Wt, C, lo, hi):
        return rng.standard_normal((Bt, Ht, Wt, C)).astype(np.float32), rng.uniform(lo, hi, (B, H, W, 2)).astype(np.float32)

    if name == "b1_wide":                   # B = 1, odd non-square texture, uv outside [0, 1] and negative
        return make(1, 16, 16, 1, 5, 7, 3, -3.0, 4.0)
    if name == "b8_shared_c4":              # B = 8, one texture for all, the float4 path
        return make(8, 12, 10, 1, 8, 8, 4, -0.5, 1.5)
    if name == "b8_own_c1":                 # B = 8, a texture per image, one channel
        return make(8, 12, 10, 8, 3, 9, 1, -2.0, 3.0)
    if name == "one_texel":                 # a 1 x 1 texture: every tap is the same texel
        return make(2, 9, 9, 2, 1, 1, 4, -2.0, 3.0)
    if name == "c7":                        # more than four channels: two channel groups
        return make(2, 8, 8, 1, 4, 6, 7, -1.0, 2.0)
    if name == "constant_uv":               # 2048 pixels on one texel cell: the wave-wide sum
        tex, uv = make(2, 32, 32, 1, 6, 4, 3, 0.0, 1.0)
        uv[...] = np.float32([0.62, 0.4])
        return tex, uv
    if name == "far":                       # far outside: exact integers above 2^24, beyond int32, and non-finite coordinates
        tex, uv = make(1, 8, 8, 1, 4, 4, 3, -1.0, 2.0)
        uv[0, 0] = np.float32([[1e6, -1e6], [-3e7, 5e7], [1e12, -1e12], [3e38, -3e38], [np.nan, 0.5], [0.5, np.inf], [-np.inf, np.nan],
                               [123456.7, -7654.3]])
        return tex, uv
    if name == "interpolated":
        return rng.standard_normal((1, 6, 5, 3)).astype(np.float32), _interpolated_uv()
    raise KeyError(name)


CASES = ["b1_wide", "b8_shared_c4", "b8_own_c1", "one_texel", "c7", "constant_uv", "far", "interpolated"]


def _run(tex, uv, g, filt, boundary):
    import largesteps.render as dr
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
    out = dr.texture(t, c, filter_mode=filt, boundary_mode=boundary)
    (out * dev(g)).sum().backward()
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), c.grad.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("filt,boundary", MODES)
def test_native_matches_statement(filt, boundary, name):
    tex, uv = _case(name)
    g = np.random.default_rng(1).standard_normal(uv.shape[:3] + (tex.shape[3],)).astype(np.float32)
    out, gt, gc = _run(tex, uv, g, filt, boundary)
    r = ts.texture(tex, uv, g, filt, boundary)
    e_out = np.abs(out - r.out).max()
    b_out = 16 * U * np.abs(tex).max()
    e_t = np.abs(gt - r.grad_tex)
    b_t = (r.grad_tex_n[..., None] + 16) * U * r.grad_tex_abs
    e_c = np.abs(gc - r.grad_uv)
    b_c = (r.grad_uv_n + 16) * U * r.grad_uv_abs
    print(f"{name} {filt} {boundary}: forward {e_out:.3e} (bound {b_out:.3e}); grad_tex worst err/bound "
          f"{(e_t / np.maximum(b_t, 1e-300)).max():.3f}, max terms {r.grad_tex_n.max()}; grad_uv worst err/bound "
          f"{(e_c / np.maximum(b_c, 1e-300)).max():.3f}")
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(gt)) and np.all(np.isfinite(gc))
    assert e_out <= b_out
    assert np.all(e_t <= b_t)
    assert np.all(e_c <= b_c)
    if name == "constant_uv":
        assert r.grad_tex_n.max() == 2048


def _parent_texture(tex, uv):
    """the lookup as it was before the kernel: plain torch, linear + wrap (the dozen lines of the parent commit, verbatim)"""
    with torch.no_grad():
        Ht, Wt = tex.shape[1], tex.shape[2]
        x = uv[..., 0] * Wt - 0.5
        y = uv[..., 1] * Ht - 0.5
        x0, y0 = torch.floor(x), torch.floor(y)
        fx, fy = (x - x0)[..., None], (y - y0)[..., None]
        i0 = torch.remainder(x0.long(), Wt)
        j0 = torch.remainder(y0.long(), Ht)
        i1, j1 = torch.remainder(i0 + 1, Wt), torch.remainder(j0 + 1, Ht)
        B = uv.shape[0]
        t = tex if tex.shape[0] == B else tex.expand(B, *tex.shape[1:])
        bi = torch.arange(B, device=uv.device).view(B, *([1] * (uv.dim() - 2)))
        t00, t10 = t[bi, j0, i0], t[bi, j0, i1]
        t01, t11 = t[bi, j1, i0], t[bi, j1, i1]
        top = t00 + (t10 - t00) * fx
        bot = t01 + (t11 - t01) * fx
        return top + (bot - top) * fy


def test_linear_wrap_forward_is_the_parents_bit_for_bit():
    import largesteps.render as dr
    golden = np.load(os.path.join(HERE, "golden", "reference_render.npz"))
    pairs = [_case(n) for n in ("b1_wide", "b8_shared_c4", "b8_own_c1", "one_texel", "c7", "interpolated")]
    pairs.append((golden["sh_envmap"][None], golden["bg_uvs"]))
    rng = np.random.default_rng(8)
    pairs.append((rng.standard_normal((1, 64, 128, 4)).astype(np.float32), rng.uniform(-4, 5, (3, 96, 80, 2)).astype(np.float32)))
    for tex, uv in pairs:
        t, c = dev(tex), dev(uv)
        got = dr.texture(t, c)
        want = _parent_texture(t, c)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want), (tex.shape, uv.shape, (got - want).abs().max().item())
        assert torch.equal(dr.texture(t, c, filter_mode="auto"), want)


def test_renderer_backgrounds_are_the_parents_bit_for_bit():
    from largesteps.render import NVDRenderer
    from test_render_gpu import scene_params
    params = scene_params(3, res=48)
    r = NVDRenderer(params)
    want = _parent_texture((params["envmap_scale"] * params["envmap"])[None], r.background_uvs()).flip(1)
    want[..., -1] = 0
    assert torch.equal(r.bgs, want)


def test_gradients_exist_and_every_mode_runs():
    """fails on the parent: its texture ran under no_grad and knew linear + wrap only"""
    import largesteps.render as dr
    tex, uv = _case("b1_wide")
    t = dev(tex).requires_grad_(True)
    out = dr.texture(t, dev(uv))
    assert out.requires_grad and out.grad_fn is not None
    for filt, boundary in MODES:
        o = dr.texture(dev(tex), dev(uv), filter_mode=filt, boundary_mode=boundary)
        assert o.shape == (1, 16, 16, 3) and not o.requires_grad
    c = dev(uv).requires_grad_(True)
    assert dr.texture(dev(tex), c).grad_fn is not None
    # a view that is neither contiguous nor 16-byte aligned takes the same path
    big = dev(np.random.default_rng(0).standard_normal((1, 5, 7, 5)).astype(np.float32))
    assert torch.equal(dr.texture(big[..., 1:5], dev(uv)), dr.texture(big[..., 1:5].contiguous(), dev(uv)))
    flat = dev(np.random.default_rng(0).uniform(-1, 2, 16 * 16 * 2 + 1).astype(np.float32))
    odd = flat[1:].view(1, 16, 16, 2)
    assert torch.equal(dr.texture(dev(tex), odd), dr.texture(dev(tex), odd.clone()))


def test_two_runs_and_cached_order_are_bitwise_identical():
    import largesteps.render as dr
    for name in ("b8_shared_c4", "constant_uv", "b8_own_c1"):
        tex, uv = _case(name)
        g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (tex.shape[3],)).astype(np.float32)
        for filt, boundary in MODES:
            a = _run(tex, uv, g, filt, boundary)
            b = _run(tex, uv, g, filt, boundary)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            # one uv tensor used twice: the second backward takes the cached order
            t, c, gg = dev(tex).requires_grad_(True), dev(uv), dev(g)
            (dr.texture(t, c, filter_mode=filt, boundary_mode=boundary) * gg).sum().backward()
            slot = c._largesteps_texel_order
            assert slot.order is not None
            first, t.grad = t.grad.clone(), None
            (dr.texture(t, c, filter_mode=filt, boundary_mode=boundary) * gg).sum().backward()
            assert c._largesteps_texel_order is slot
            assert torch.equal(t.grad, first) and np.array_equal(first.cpu().numpy(), a[1])


def test_changing_uv_in_place_invalidates_the_cached_order():
    import largesteps.render as dr
    tex, uv = _case("b1_wide")
    g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (3,)).astype(np.float32)
    t, c, gg = dev(tex).requires_grad_(True), dev(uv), dev(g)
    (dr.texture(t, c) * gg).sum().backward()
    slot = c._largesteps_texel_order
    c.add_(0.37)
    t.grad = None
    (dr.texture(t, c) * gg).sum().backward()
    assert c._largesteps_texel_order is not slot
    assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), g, "linear", "wrap")[1])
    # another mode on the same tensor is another order
    t.grad = None
    (dr.texture(t, c, boundary_mode="clamp") * gg).sum().backward()
    assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), g, "linear", "clamp")[1])


def test_captured_forward_and_backward_match_eager():
    import largesteps.render as dr
    from largesteps.capture import CapturedStep
    tex, uv = _case("b8_shared_c4")
    g = dev(np.random.default_rng(2).standard_normal(uv.shape[:3] + (4,)).astype(np.float32))
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)

    def body():
        t.grad = c.grad = None
        out = dr.texture(t, c, boundary_mode="clamp")
        (out * g).sum().backward()
        return out, t.grad, c.grad

    step = CapturedStep(body)
    for it in range(4):
        with torch.no_grad():
            t.mul_(0.9).add_(0.01 * it)             # the texture is updated in place between replays, as an optimizer would
            if it == 2:
                c.add_(0.123)                       # and once the coordinates too: the replay sorts what it finds
        got = [x.clone() for x in step()]
        t2, c2 = t.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
        out = dr.texture(t2, c2, boundary_mode="clamp")
        (out * g).sum().backward()
        for x, y in zip(got, (out.detach(), t2.grad, c2.grad)):
            assert torch.equal(x, y), it


def _chain_statement(pos, f, attr, tex, H, W):
    """rasterize -> interpolate(uv attribute) -> texture -> antialias by the statements: (rast, texture namespace, image)"""
    rast = rs.rasterize(pos, f, H, W)
    uv = rs.interpolate(attr, rast, f)
    r = ts.texture(tex, uv, None, "linear", "wrap", coords=np.float64)
    return rast, r, rs.antialias(r.out, rast, pos, f).astype(np.float64)


def _chain_device(tp, tf, ta, tt, H, W):
    import largesteps.render as dr
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    uv = dr.interpolate(ta, rast, tf)[0]
    return dr.antialias(dr.texture(tt, uv), rast, tp, tf)


def test_chain_gradients_match_finite_differences_of_the_statements():
    """rasterize -> interpolate(uv) -> texture -> antialias -> loss on a small icosphere: the device's gradient to the texture and to
    the clip-space positions against central differences of the statements in random directions (z excluded: its gradient is dropped),
    with the method, step and tolerances of test_render_gpu.test_gradients_match_finite_differences. Only pixels whose triangle AND
    whose base tap are the same in the three renders are summed: the image has a jump where a pixel changes triangle at a silhouette
    and a kink where uv crosses a texel centre line."""
    pos, f, H, W = scene("sphere")
    rng = np.random.default_rng(7)
    attr = (0.5 + 0.9 * pos[0, :, :2] / np.abs(pos[0, :, :2]).max()).astype(np.float32)
    tex = rng.uniform(0, 1, (1, 6, 5, 3)).astype(np.float32)
    g = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    eps = 2e-4
    r0, x0, _ = _chain_statement(pos, f, attr, tex, H, W)
    for trial in range(4):
        d = rng.standard_normal(pos.shape).astype(np.float32)
        d[..., 2] = 0
        dt = rng.standard_normal(tex.shape).astype(np.float32)
        rp, xp, ip = _chain_statement(pos + np.float32(eps) * d, f, attr, tex, H, W)
        rm, xm, im = _chain_statement(pos - np.float32(eps) * d, f, attr, tex, H, W)
        keep = (rp[..., 3] == r0[..., 3]) & (rm[..., 3] == r0[..., 3]) & (r0[..., 3] > 0)
        keep &= (xp.i0 == x0.i0) & (xm.i0 == x0.i0) & (xp.j0 == x0.j0) & (xm.j0 == x0.j0)
        assert keep.sum() > 0.5 * (r0[..., 3] > 0).sum()
        w = g * keep[..., None]
        fd_pos = float(((ip - im) * w).sum() / (2 * eps))
        tp_, tm_ = (_chain_statement(pos, f, attr, tex + s * np.float32(eps) * dt, H, W)[2] for s in (1, -1))
        fd_tex = float(((tp_ - tm_) * w).sum() / (2 * eps))
        tp, tt = dev(pos).requires_grad_(True), dev(tex).requires_grad_(True)
        (_chain_device(tp, dev(f), dev(attr), tt, H, W) * dev(w.astype(np.float32))).sum().backward()
        an_pos = float((tp.grad.double() * dev(d).double()).sum())
        an_tex = float((tt.grad.double() * dev(dt).double()).sum())
        print(f"trial {trial}: kept {keep.sum()} pixels; pos fd {fd_pos:.6f} an {an_pos:.6f}; tex fd {fd_tex:.6f} an {an_tex:.6f}")
        assert abs(an_pos) > 1.0 and abs(fd_pos - an_pos) <= 0.03 * abs(an_pos), ("pos", trial, fd_pos, an_pos)
        assert abs(an_tex) > 1.0 and abs(fd_tex - an_tex) <= 0.03 * abs(an_tex), ("tex", trial, fd_tex, an_tex)
