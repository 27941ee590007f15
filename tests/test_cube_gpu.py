"""
largesteps.render.texture(..., boundary_mode='cube') on the device against tests/cube_statement.py (the numpy specification) with derived
bounds, against the 2-D lookup of the face (bit for bit, for pixels whose taps stay inside it), against itself (two runs, cached and
fresh item order, captured and eager), and through the chain rasterize -> interpolate -> texture(cube) -> antialias against central
differences of the statements.

Bounds (u = 2^-24, the unit roundoff of fp32; the statement shares the device's fp32 coordinates and fractions -- sc / |ma|, s, x, fx
are the same numbers -- and continues in fp64):
  forward    |err| <= 16 u max|tex|. No dropped tap: (t10 - t00), * fx, + t00 for top and for bot, then (bot - top), * fy, + top: nine
             roundings, each of a quantity of at most 2 max|tex|. With a dropped tap, out = sum w'_k t_k: 1 - fx, 1 - fy, their product,
             w_c / 3 and the addition of the third are at most five relative roundings of a weight, the product with the texel a
             sixth, two additions: eight roundings of quantities of at most sum w'_k |t_k| <= max|tex|. Nearest: exact.
  grad_tex   an entry that sums n terms g w'_tap: |err| <= (n + 16) u S, S the sum of the terms' absolute values: n - 1 additions and
             at most six roundings inside a term (the five of a weight, times g).
  grad_uv    per component (4 C + 16) u S + 16 * 2^-149, S the statement's sum of absolute values (the terms are the 4 C products
             g * texel * weight): C - 1 additions over the channels and one per channel group (fewer than 4 C in all), and inside a term
             the mean of three texels for a dropped tap (two additions, a division), the texel difference, 1 - f, the product, the
             sum of the two products, times g, times n, the division by |ma|, and for the major-axis component the product with
             sc / |ma| and one more addition: thirteen. The absolute part: a direction of length 3e38 has a gradient near the smallest
             normal number, where an operation rounds to a multiple of 2^-149 and not relatively.
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

import cube_cases as cc  # noqa: E402
import cube_statement as cs  # noqa: E402
import render_statement as rs  # noqa: E402
from render_scenes import scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = 2.0 ** -24
TINY = 16 * 2.0 ** -149


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sphere_directions():
    """(pos, f, attr (V, 3), H, W): the sphere scene with its own vertex positions as the direction attribute"""
    pos, f, H, W = scene("sphere")
    attr = np.ascontiguousarray(pos[0, :, :3] - pos[0, :, :3].mean(0)).astype(np.float32)
    return pos, f, attr, H, W


def _interpolated_directions():
    """uv (1, H, W, 3) from a real rasterize -> interpolate of a 3-channel attribute (background pixels: the zero vector, no face)"""
    import largesteps.render as dr
    pos, f, attr, H, W = _sphere_directions()
    rast = dr.rasterize(None, dev(pos), dev(f), (H, W))[0]
    return dr.interpolate(dev(attr), rast, dev(f))[0].cpu().numpy()


def _case(name, filt="linear"):
    """(tex, uv) fp32 arrays. Only `threshold` depends on the filter (pixels inside cells, or on texel centres)"""
    rng = np.random.default_rng(sum(map(ord, name)))

    def make(B, H, W, Bt, n, C):
        return rng.standard_normal((Bt, 6, n, n, C)).astype(np.float32), rng.standard_normal((B, H, W, 3)).astype(np.float32)

    if name == "n1_b2":                     # one texel a face: every linear tap but one folds or is dropped
        return make(2, 9, 9, 2, 1, 3)
    if name == "n2":
        return make(1, 16, 16, 1, 2, 2)
    if name == "n5_c3_shared_b8":
        return make(8, 12, 10, 1, 5, 3)
    if name == "n8_c4_own":                 # the float4 path
        return make(4, 12, 10, 4, 8, 4)
    if name == "c7":                        # two channel groups
        return make(2, 8, 8, 1, 4, 7)
    if name == "c32":
        return make(1, 8, 8, 1, 3, 32)
    if name == "seams":                     # within 0.3 texels of all 12 edges (from both sides) and all 8 corners; and exactly on them
        tex = rng.standard_normal((1, 6, 5, 5, 3)).astype(np.float32)
        d = cc.directions_inside_cells(rng, 5, True, per_face=8, per_border=24)[0, 0]
        ties = np.array([[sa if k == a else sb if k == b else t for k in range(3)] for a, b in ((0, 1), (0, 2), (1, 2))
                         for sa in (1.0, -1.0) for sb in (1.0, -1.0) for t in (-1.0, -0.6, 0.0, 0.25, 1.0)])
        return tex, np.concatenate([d, ties, 3.0 * ties]).astype(np.float32)[None, None]
    if name == "constant":                  # 2048 pixels with one direction: the wave-wide sum
        tex, uv = make(2, 32, 32, 1, 4, 3)
        uv[...] = np.float32([0.3, -0.9, 0.5])
        return tex, uv
    if name == "threshold":                 # 63 / 64 / 65 / 129 items on single texels, border texels that collect from two faces
        n = cc.THRESHOLD_N
        return rng.standard_normal((1, 6, n, n, 3)).astype(np.float32), cc.threshold_directions(rng, filt == "linear")
    if name == "far":                       # lengths 1e-30 .. 3e38, exact ties, and directions without a face
        tex, uv = make(1, 8, 16, 1, 4, 3)
        uv /= np.abs(uv).max(-1, keepdims=True)
        uv *= (10.0 ** rng.uniform(-30, 38.47, uv.shape[:3]))[..., None].astype(np.float32)
        uv[0, 0, :8] = np.float32([[3e38, -3e38, 3e38], [1e-30, 1e-30, -1e-30], [2.5, -2.5, 1.0], [0.0, 7.0, -7.0], [np.nan, 1, 0],
                                   [1, np.inf, 0], [0, 0, -np.inf], [0, 0, 0]])
        uv[0, 1, :3] = np.float32([[-0.0, 0.0, -0.0], [-1e30, 1e30, 1e30], [3e38, 1e-30, -1e-30]])
        return tex, uv
    if name == "interpolated":
        return rng.standard_normal((1, 6, 6, 6, 3)).astype(np.float32), _interpolated_directions()
    raise KeyError(name)


CASES = ["n1_b2", "n2", "n5_c3_shared_b8", "n8_c4_own", "c7", "c32", "seams", "constant", "threshold", "far", "interpolated"]


def _run(tex, uv, g, filt):
    import largesteps.render as dr
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
    out = dr.texture(t, c, filter_mode=filt, boundary_mode="cube")
    (out * dev(g)).sum().backward()
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), c.grad.cpu().numpy()


def check_against_statement(name, tex, uv, g, filt):
    """the comparison of tests/test_cube_gpu.py and tests/test_cube_scale_gpu.py: returns the statement's namespace"""
    out, gt, gc = _run(tex, uv, g, filt)
    r = cs.cube(tex, uv, g, filt)
    e_out = np.abs(out - r.out).max()
    b_out = 16 * U * np.abs(tex).max()
    e_t = np.abs(gt - r.grad_tex)
    b_t = (r.grad_tex_n[..., None] + 16) * U * r.grad_tex_abs
    e_c = np.abs(gc - r.grad_uv)
    b_c = (r.grad_uv_n + 16) * U * r.grad_uv_abs + TINY
    print(f"{name} {filt}: forward {e_out:.3e} (bound {b_out:.3e}); grad_tex worst err/bound "
          f"{(e_t / np.maximum(b_t, 1e-300)).max():.3f}, max terms {r.grad_tex_n.max()}; grad_uv worst err/bound {(e_c / b_c).max():.3f}")
    assert out.shape == r.out.shape and gt.shape == tex.shape and gc.shape == uv.shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(gt)) and np.all(np.isfinite(gc))
    assert e_out <= b_out
    assert np.all(e_t <= b_t)
    assert np.all(e_c <= b_c)
    assert np.all(out[~r.finite] == 0) and np.all(gc[~r.finite] == 0)
    if filt == "nearest":
        assert not gc.any() and np.array_equal(out, r.out.astype(np.float32))
    return r


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("filt", cs.FILTERS)
def test_native_matches_statement(filt, name):
    tex, uv = _case(name, filt)
    g = np.random.default_rng(1).standard_normal(uv.shape[:3] + (tex.shape[4],)).astype(np.float32)
    r = check_against_statement(name, tex, uv, g, filt)
    linear = filt == "linear"
    if name == "n1_b2" and linear:
        assert (r.drop >= 0).all()
    if name == "seams" and linear:
        assert set(r.face.ravel()) == set(range(6)) and (r.drop >= 0).sum() >= 6 * 24 and (~r.inside & (r.drop < 0)).sum() >= 6 * 48
    if name == "constant":
        assert r.grad_tex_n.max() == 2048
    if name == "threshold":
        counts = set(r.grad_tex_n.ravel().tolist())
        assert {63, 64, 65, 129} <= counts
        if linear:                          # the border texels of +x collect 25 items of their own face and 40 across the edge from +z
            assert r.grad_tex_n[0, 0, 3, 0] == 65 and r.grad_tex_n[0, 0, 4, 0] == 65 and r.grad_tex_n[0, 0, 3, 1] == 25
            assert r.grad_tex_n[0, 4, 3, 7] == 40 and r.grad_tex_n.sum() == 4 * uv.shape[2]
    if name == "far":
        assert (~r.finite).sum() == 5 and np.abs(uv[r.finite]).max() >= 3e38 and np.abs(uv[r.finite]).max(-1).min() <= 1e-29
    if name == "interpolated":
        assert 0.2 < r.finite.mean() < 0.9 and len(set(r.face[r.finite].ravel())) >= 3


def test_pixels_inside_a_face_are_the_2d_lookup_bit_for_bit():
    """a pixel whose four taps lie inside its face is texture(tex[:, f], (s, t), 'linear', 'clamp'), (s, t) computed in torch fp32 by the
    rules: one division, one add, one multiply. Nearest: the same with 'nearest' (s n < n but for s = 1, which clamp maps to n - 1)."""
    import largesteps.render as dr
    for name in ("n5_c3_shared_b8", "n8_c4_own", "c7", "interpolated"):
        tex, uv = _case(name)
        t, d = torch.from_numpy(tex), torch.from_numpy(uv)
        r = cs.cube(tex, uv, None, "linear")
        x, y, z = d.unbind(-1)
        table = [(-z, -y, x), (z, -y, x), (x, z, y), (x, -z, y), (x, -y, z), (-x, -y, z)]
        for filt in cs.FILTERS:
            got = dr.texture(dev(tex), dev(uv), filter_mode=filt, boundary_mode="cube").cpu()
            seen = 0
            for f, (sc, tc, ma) in enumerate(table):
                st = torch.stack([(sc / ma.abs() + 1.0) * 0.5, (tc / ma.abs() + 1.0) * 0.5], dim=-1)
                sel = torch.from_numpy((r.face == f) & (r.inside if filt == "linear" else r.finite))
                st = torch.where(sel[..., None], st, torch.zeros(()))                   # (elsewhere: any finite coordinate)
                want = dr.texture(dev(tex[:, f]), st.to(DEV), filter_mode=filt, boundary_mode="clamp").cpu()
                assert torch.equal(got[sel], want[sel]), (name, filt, f)
                seen += int(sel.sum())
            assert seen > 0.15 * r.finite.sum()


def test_argument_errors_on_the_device():
    import largesteps.render as dr
    cube, dirs = torch.zeros(1, 6, 4, 4, 3, device=DEV), torch.zeros(2, 5, 5, 3, device=DEV)
    assert dr.texture(cube, dirs, boundary_mode="cube").shape == (2, 5, 5, 3)
    assert dr.texture(cube, dirs, filter_mode="auto", boundary_mode="cube").shape == (2, 5, 5, 3)
    with pytest.raises(NotImplementedError, match="HIP device"):
        dr.texture(cube.cpu(), dirs, boundary_mode="cube")
    with pytest.raises(TypeError):
        dr.texture(cube.double(), dirs, boundary_mode="cube")
    with pytest.raises(TypeError):
        dr.texture(cube, dirs.half(), boundary_mode="cube")
    for bad in (cube[0], cube[:, :5], cube[:, :, :3], torch.zeros(1, 4, 4, 3, device=DEV)):
        with pytest.raises(ValueError, match="cube map"):
            dr.texture(bad, dirs, boundary_mode="cube")
    for bad in (dirs[..., :2], dirs[0], torch.zeros(2, 5, 5, 4, device=DEV)):
        with pytest.raises(ValueError, match="directions"):
            dr.texture(cube, bad, boundary_mode="cube")
    with pytest.raises(ValueError, match="batches"):
        dr.texture(cube.expand(3, -1, -1, -1, -1), dirs, boundary_mode="cube")
    with pytest.raises(ValueError, match="channels"):
        dr.texture(torch.zeros(1, 6, 2, 2, 33, device=DEV), dirs, boundary_mode="cube")
    with pytest.raises(ValueError, match="empty"):
        dr.texture(cube, dirs[:, :0], boundary_mode="cube")
    with pytest.raises(ValueError, match="filter_mode"):
        dr.texture(cube, dirs, filter_mode="cubic", boundary_mode="cube")
    for mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        with pytest.raises(NotImplementedError, match="mipmapped cube maps"):
            dr.texture(cube, dirs, filter_mode=mode, boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="mipmapped cube maps"):
        dr.texture_construct_mip(cube, cube_mode=True)
    with pytest.raises(OverflowError):
        dr.texture(cube, torch.zeros(1, 1, 1, 3, device=DEV).expand(1, 1 << 15, 1 << 14, 3), boundary_mode="cube")
    # views that are neither contiguous nor aligned take the same path
    rng = np.random.default_rng(0)
    big = dev(rng.standard_normal((1, 6, 4, 4, 5)).astype(np.float32))
    flat = dev(rng.standard_normal(2 * 5 * 5 * 3 + 1).astype(np.float32))
    odd = flat[1:].view(2, 5, 5, 3)
    assert torch.equal(dr.texture(big[..., 1:5], odd, boundary_mode="cube"), dr.texture(big[..., 1:5].contiguous(), odd.clone(), boundary_mode="cube"))


def test_two_runs_and_cached_order_are_bitwise_identical():
    import largesteps.render as dr
    for name in ("n5_c3_shared_b8", "constant", "n8_c4_own", "seams"):
        tex, uv = _case(name)
        g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (tex.shape[4],)).astype(np.float32)
        for filt in cs.FILTERS:
            a = _run(tex, uv, g, filt)
            b = _run(tex, uv, g, filt)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            # one uv tensor used twice: the second backward takes the cached order
            t, c, gg = dev(tex).requires_grad_(True), dev(uv), dev(g)
            (dr.texture(t, c, filter_mode=filt, boundary_mode="cube") * gg).sum().backward()
            slot = c._largesteps_cube_order
            assert slot.order is not None and slot.order.numel() == (4 if filt == "linear" else 1) * uv[..., 0].size
            assert slot.key == (c._version, c.data_ptr(), tuple(c.shape), tuple(c.stride()), tex.shape[0], tex.shape[2], int(filt == "linear"))
            first, t.grad = t.grad.clone(), None
            (dr.texture(t, c, filter_mode=filt, boundary_mode="cube") * gg).sum().backward()
            assert c._largesteps_cube_order is slot
            assert torch.equal(t.grad, first) and np.array_equal(first.cpu().numpy(), a[1])
    # changing uv in place, or another filter on the same tensor, is another order
    tex, uv = _case("n5_c3_shared_b8")
    g = np.random.default_rng(2).standard_normal(uv.shape[:3] + (3,)).astype(np.float32)
    t, c, gg = dev(tex).requires_grad_(True), dev(uv), dev(g)
    (dr.texture(t, c, boundary_mode="cube") * gg).sum().backward()
    slot = c._largesteps_cube_order
    c.mul_(-1.0).add_(0.37)
    t.grad = None
    (dr.texture(t, c, boundary_mode="cube") * gg).sum().backward()
    assert c._largesteps_cube_order is not slot
    assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), g, "linear")[1])
    t.grad = None
    (dr.texture(t, c, filter_mode="nearest", boundary_mode="cube") * gg).sum().backward()
    assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), g, "nearest")[1])


def test_captured_forward_and_backward_match_eager():
    import largesteps.render as dr
    from largesteps.capture import CapturedStep
    tex, uv = _case("n8_c4_own")
    g = dev(np.random.default_rng(2).standard_normal(uv.shape[:3] + (4,)).astype(np.float32))
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)

    def body():
        t.grad = c.grad = None
        out = dr.texture(t, c, boundary_mode="cube")
        (out * g).sum().backward()
        return out, t.grad, c.grad

    step = CapturedStep(body)
    for it in range(4):
        with torch.no_grad():
            t.mul_(0.9).add_(0.01 * it)             # the cube is updated in place between replays, as an optimizer would
            if it >= 2:
                c.add_(0.123 * it)                  # and the directions too: the replay sorts what it finds
        got = [x.clone() for x in step()]
        t2, c2 = t.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
        out = dr.texture(t2, c2, boundary_mode="cube")
        (out * g).sum().backward()
        for x, y in zip(got, (out.detach(), t2.grad, c2.grad)):
            assert torch.equal(x, y), it


def _chain_statement(pos, f, attr, tex, H, W):
    """rasterize -> interpolate(direction attribute) -> texture(cube) -> antialias by the statements: (directions, cube namespace, image)"""
    rast = rs.rasterize(pos, f, H, W)
    d = rs.interpolate(attr, rast, f)
    r = cs.cube(tex, d, None, "linear", coords=np.float64)
    return d, r, rs.antialias(r.out, rast, pos, f).astype(np.float64)


def test_chain_gradients_match_finite_differences_of_the_statements():
    """rasterize -> interpolate(directions) -> texture(cube) -> antialias -> loss on a small icosphere: the device's gradient to the
    direction attribute and to the cube against central differences of the statements in random directions, with the method, step and
    tolerances of test_texture_gpu.test_chain_gradients_match_finite_differences_of_the_statements. Only pixels whose face and base tap
    are the same in the three renders are summed: the lookup has a kink where a direction crosses a texel centre line or a seam."""
    import largesteps.render as dr
    pos, f, attr, H, W = _sphere_directions()
    rng = np.random.default_rng(7)
    tex = rng.uniform(0, 1, (1, 6, 4, 4, 3)).astype(np.float32)
    g = rng.standard_normal((1, H, W, 3)).astype(np.float32)
    eps = 2e-4
    d0, x0, _ = _chain_statement(pos, f, attr, tex, H, W)
    covered = x0.finite
    scale = np.abs(attr).max()
    for trial in range(4):
        da = (scale * rng.standard_normal(attr.shape)).astype(np.float32)
        _, xp, ip = _chain_statement(pos, f, attr + np.float32(eps) * da, tex, H, W)
        _, xm, im = _chain_statement(pos, f, attr - np.float32(eps) * da, tex, H, W)
        keep = covered & (xp.face == x0.face) & (xm.face == x0.face)
        keep &= (xp.i0 == x0.i0) & (xm.i0 == x0.i0) & (xp.j0 == x0.j0) & (xm.j0 == x0.j0)
        assert keep.sum() > 0.5 * covered.sum()
        w = g * keep[..., None]
        # a step of the cube along which the loss does change: the signs of the statement's own gradient of the lookup (before the
        # antialiasing), blurred by noise -- a purely random step often sums to nearly nothing over 96 texels
        dt = (np.sign(cs.cube(tex, d0, w, "linear", coords=np.float64).grad_tex) + 0.5 * rng.standard_normal(tex.shape)).astype(np.float32)
        fd_attr = float(((ip - im) * w).sum() / (2 * eps))
        tp_, tm_ = (_chain_statement(pos, f, attr, tex + s * np.float32(eps) * dt, H, W)[2] for s in (1, -1))
        fd_tex = float(((tp_ - tm_) * w).sum() / (2 * eps))
        ta, tt, tp, tf = dev(attr).requires_grad_(True), dev(tex).requires_grad_(True), dev(pos), dev(f)
        rast = dr.rasterize(None, tp, tf, (H, W))[0]
        col = dr.texture(tt, dr.interpolate(ta, rast, tf)[0], boundary_mode="cube")
        (dr.antialias(col, rast, tp, tf) * dev(w.astype(np.float32))).sum().backward()
        an_attr = float((ta.grad.double() * dev(da).double()).sum())
        an_tex = float((tt.grad.double() * dev(dt).double()).sum())
        print(f"trial {trial}: kept {keep.sum()} of {covered.sum()} pixels; attr fd {fd_attr:.6f} an {an_attr:.6f}; tex fd {fd_tex:.6f} an {an_tex:.6f}")
        assert abs(an_attr) > 1.0 and abs(fd_attr - an_attr) <= 0.03 * abs(an_attr), ("attr", trial, fd_attr, an_attr)
        assert abs(an_tex) > 1.0 and abs(fd_tex - an_tex) <= 0.03 * abs(an_tex), ("tex", trial, fd_tex, an_tex)
