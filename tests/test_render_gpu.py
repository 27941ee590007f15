"""
largesteps.render on the device against tests/render_statement.py (the numpy specification), finite differences, itself (two runs),
and the reference's whole optimisation loop (eager, captured, and end to end on a synthetic scene).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import render_statement as rs  # noqa: E402
from render_scenes import SCENES, look_at, scene  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def to_dev(pos, f, dtype=torch.int64):
    return torch.from_numpy(pos).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV, dtype)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", SCENES)
def test_rasterize_matches_statement(name):
    import largesteps.render as dr
    pos, f, H, W = scene(name)
    tp, tf = to_dev(pos, f)
    rast, db = dr.rasterize(dr.RasterizeGLContext(), tp, tf, (H, W))
    got = rast.cpu().numpy()
    ref = rs.rasterize(pos, f, H, W)
    assert np.array_equal(got[..., 3], ref[..., 3]), f"{name}: triangle ids differ at {np.argwhere(got[..., 3] != ref[..., 3])[:5]}"
    assert ulps(got[..., :3], ref[..., :3]).max() <= 1, f"{name}: u, v, z/w beyond 1 ulp"
    covered = (ref[..., 3] > 0).mean()
    if name == "empty":
        assert covered == 0
    elif name == "quad":
        assert covered == 1.0
    else:
        assert 0.02 < covered < 1.0
    assert torch.count_nonzero(db) == 0


def _loss_weights(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("name", ["sphere", "sphere_b3", "folded", "near_plane"])
def test_interpolate_and_antialias_match_statement(name):
    import largesteps.render as dr
    pos, f, H, W = scene(name)
    B, V = pos.shape[0], pos.shape[1]
    attr = np.random.default_rng(2).uniform(0, 1, (1, V, 3)).astype(np.float32)
    tp, tf = to_dev(pos, f)
    tp.requires_grad_(True)
    ta = torch.from_numpy(attr).to(DEV).requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    col = dr.interpolate(ta, rast, tf)[0]
    col.retain_grad()
    out = dr.antialias(col, rast, tp, tf, pos_gradient_boost=2.0)
    g = _loss_weights(out.shape, 3)
    (out * g).sum().backward()
    r = rast.detach().cpu().numpy()
    c_ref = rs.interpolate(attr, r, f)
    assert np.abs(col.detach().cpu().numpy() - c_ref).max() <= 1e-6
    o_ref = rs.antialias(col.detach().cpu().numpy(), r, pos, f)
    assert np.abs(out.detach().cpu().numpy() - o_ref).max() <= 2e-6
    gn = g.cpu().numpy()
    gc_ref, gp_aa = rs.antialias_backward(col.detach().cpu().numpy(), r, pos, f, gn, boost=2.0)
    np.testing.assert_allclose(col.grad.cpu().numpy(), gc_ref, rtol=1e-5, atol=1e-5)
    ga_ref, gr_ref = rs.interpolate_backward(attr, r, f, gc_ref)
    np.testing.assert_allclose(ta.grad.cpu().numpy(), ga_ref, rtol=1e-4, atol=1e-4)
    gp_ref = gp_aa + rs.rasterize_backward(pos, f, r, gr_ref)
    scale = np.abs(gp_ref).max()
    assert np.abs(tp.grad.cpu().numpy() - gp_ref).max() <= 2e-4 * max(scale, 1.0)
    assert np.all(tp.grad.cpu().numpy()[..., 2] == 0)


def _aa_loss(tp, tf, attr, g, H, W):
    import largesteps.render as dr
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    col = dr.interpolate(attr, rast, tf)[0]
    return (dr.antialias(col, rast, tp, tf) * g).sum()


def _interp(tp, tf, attr, H, W):
    import largesteps.render as dr
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    return rast, dr.interpolate(attr, rast, tf)[0]


def test_gradients_match_finite_differences():
    """Central differences of image losses in random directions of all clip-space positions (z excluded: its gradient is dropped).
    (a) a constant colour through antialias on a sheet whose silhouette is its boundary: the image is continuous in the positions
    (away from the moment a centre is crossed near a silhouette vertex, or an edge turns into a silhouette edge: neither happens within
    these steps);
    (b) a varying attribute through interpolate, summed over the pixels whose triangle is the same in the three renders (antialias
    is continuous in the silhouette only up to the colour difference across one pixel, 0.5 |c_q - c_p| per crossed centre)."""
    pos, f, H, W = scene("sheet")
    V = pos.shape[1]
    tp, tf = to_dev(pos, f)
    rng = np.random.default_rng(7)
    ones = torch.ones((V, 3), device=DEV)
    g = _loss_weights((1, H, W, 3), 6)
    x = tp.clone().requires_grad_(True)
    _aa_loss(x, tf, ones, g, H, W).backward()
    eps = 2e-4
    for trial in range(4):
        d = torch.from_numpy(rng.standard_normal(pos.shape).astype(np.float32)).to(DEV)
        d[..., 2] = 0
        with torch.no_grad():
            fd = float((_aa_loss(tp + eps * d, tf, ones, g, H, W).double() - _aa_loss(tp - eps * d, tf, ones, g, H, W).double()) / (2 * eps))
        an = float((x.grad.double() * d.double()).sum())
        assert abs(an) > 1.0 and abs(fd - an) <= 0.03 * abs(an), ("antialias", trial, fd, an)
    pos, f, H, W = scene("sphere")
    V = pos.shape[1]
    tp, tf = to_dev(pos, f)
    attr = torch.from_numpy(rng.uniform(0, 1, (V, 3)).astype(np.float32)).to(DEV)
    g = _loss_weights((1, H, W, 3), 6)
    for trial in range(4):
        d = torch.from_numpy(rng.standard_normal(pos.shape).astype(np.float32)).to(DEV)
        d[..., 2] = 0
        with torch.no_grad():
            rp, cp = _interp(tp + eps * d, tf, attr, H, W)
            rm, cm = _interp(tp - eps * d, tf, attr, H, W)
        y = tp.clone().requires_grad_(True)
        r0, c0 = _interp(y, tf, attr, H, W)
        keep = ((rp[..., 3] == r0[..., 3]) & (rm[..., 3] == r0[..., 3]) & (r0[..., 3] > 0)).detach()[..., None].float()
        (c0 * g * keep).sum().backward()
        fd = float(((cp.double() - cm.double()) * g * keep).sum() / (2 * eps))
        an = float((y.grad.double() * d.double()).sum())
        assert abs(an) > 1.0 and abs(fd - an) <= 0.03 * abs(an), ("interpolate", trial, fd, an)


def _run_all(pos, f, attr, H, W, dtype=torch.int64, attr_shape=None):
    import largesteps.render as dr
    tp, tf = to_dev(pos, f, dtype)
    tp.requires_grad_(True)
    ta = torch.from_numpy(attr).to(DEV)
    if attr_shape is not None:
        ta = ta.reshape(attr_shape)
    ta.requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    col = dr.interpolate(ta, rast, tf)[0]
    out = dr.antialias(col, rast, tp, tf)
    (out * _loss_weights(out.shape, 9)).sum().backward()
    return [t.detach().cpu().numpy() for t in (rast, col, out, tp.grad, ta.grad)]


def test_two_runs_are_bitwise_identical_and_int32_matches_int64():
    pos, f, H, W = scene("sphere_b3")
    attr = np.random.default_rng(4).uniform(0, 1, (1, pos.shape[1], 3)).astype(np.float32)
    a = _run_all(pos, f, attr, H, W)
    b = _run_all(pos, f, attr, H, W)
    c = _run_all(pos, f, attr, H, W, dtype=torch.int32)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y)
        assert np.array_equal(x, z)


def test_full_screen_quad_and_large_batch():
    pos, f, H, W = scene("quad")
    pos = np.repeat(pos, 9, axis=0)
    pos[1:, :, :2] *= np.linspace(0.5, 3.0, 8, dtype=np.float32)[:, None, None]
    import largesteps.render as dr
    tp, tf = to_dev(pos, f)
    rast = dr.rasterize(None, tp, tf, (H, W))[0].cpu().numpy()
    assert np.array_equal(rast[..., 3], rs.rasterize(pos, f, H, W)[..., 3])
    # a 512 x 512 frame of two triangles: every pixel exactly once
    r = dr.rasterize(None, torch.from_numpy(pos[:1]).to(DEV), tf, (512, 512))[0]
    assert int((r[..., 3] > 0).sum()) == 512 * 512


def test_attr_broadcasting():
    pos, f, H, W = scene("sphere_b3")
    B, V = pos.shape[0], pos.shape[1]
    attr = np.random.default_rng(8).uniform(0, 1, (V, 2)).astype(np.float32)
    a2 = _run_all(pos, f, attr, H, W, attr_shape=(V, 2))
    a1 = _run_all(pos, f, attr, H, W, attr_shape=(1, V, 2))
    full = np.repeat(attr[None], B, axis=0)
    ab = _run_all(pos, f, full, H, W)
    for x, y in zip(a2[:4], a1[:4]):
        assert np.array_equal(x, y)
    assert a2[4].shape == (V, 2) and a1[4].shape == (1, V, 2)
    assert np.array_equal(a2[4], a1[4][0])
    np.testing.assert_allclose(ab[4].sum(0), a1[4][0], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(ab[2], a1[2])


# ---- the reference's loop -----------------------------------------------------------------------------------------------------------
def envmap(h=16, w=32):
    th = np.linspace(0, np.pi, h)[:, None]
    ph = np.linspace(0, 2 * np.pi, w)[None, :]
    r = 0.6 + 0.4 * np.cos(th) + 0.1 * np.sin(ph)
    g = 0.5 + 0.3 * np.sin(th) * np.cos(ph)
    b = 0.4 + 0.3 * np.cos(2 * th)
    return np.stack([r + 0 * ph, g + 0 * th, b + 0 * ph, np.ones((h, w))], -1).astype(np.float32)


def scene_params(n_views, res=64):
    views = []
    for k in range(n_views):
        a = 2 * np.pi * k / n_views
        el = 0.5 * np.sin(3 * a)
        views.append(torch.from_numpy(look_at((3 * np.cos(a) * np.cos(el), 3 * np.sin(el), 3 * np.sin(a) * np.cos(el)))).float().to(DEV))
    return {"res_x": res, "res_y": res, "fov": 45.0, "near_clip": 0.1, "far_clip": 100.0, "view_mats": views,
            "envmap": torch.from_numpy(envmap()).to(DEV), "envmap_scale": 1.0}


def _body_parts(shading):
    from largesteps import synthetic
    from largesteps.render import NVDRenderer
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    vt, ft = synthetic.icosphere(12)
    vt = vt * (1.0 + 0.15 * np.sin(3 * vt[:, :1]) * np.cos(2 * vt[:, 1:2]) + 0.1 * np.sin(4 * vt[:, 2:3])).astype(np.float32)
    tvt, tft = torch.from_numpy(vt.astype(np.float32)).to(DEV), torch.from_numpy(ft).to(DEV)
    renderer = NVDRenderer(scene_params(8), shading=shading)
    ref = renderer.render(tvt, compute_vertex_normals(tvt, tft, compute_face_normals(tvt, tft)), tft)
    return renderer, ref, tvt, tft


def test_captured_loop_body_matches_eager():
    from largesteps import synthetic
    from largesteps.capture import CapturedStep
    from largesteps.geometry import compute_matrix
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    from largesteps.optimize import AdamUniform
    from largesteps.parameterize import to_differential, from_differential
    renderer, ref, _, _ = _body_parts(True)
    v, f = synthetic.icosphere(6)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    M = compute_matrix(tv, tf, lambda_=10.0)

    def make():
        u = to_differential(M, tv).clone().requires_grad_(True)
        opt = AdamUniform([u], 1e-2, capturable=True)

        def body():
            x = from_differential(M, u, 'Cholesky')
            n = compute_vertex_normals(x, tf, compute_face_normals(x, tf))
            loss = (renderer.render(x, n, tf) - ref).abs().mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss
        return u, body

    u1, body1 = make()
    eager = [float(body1().detach()) for _ in range(5)]
    u2, body2 = make()
    step = CapturedStep(body2, warmup=2)
    captured = [float(step().detach()) for _ in range(3)]
    torch.cuda.synchronize()
    np.testing.assert_allclose(captured, eager[2:], rtol=1e-5)
    np.testing.assert_allclose(u2.detach().cpu().numpy(), u1.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert eager[-1] < eager[0]


def _surface_distance(v, target):
    return float(torch.cdist(v, target).min(dim=1).values.mean())


@pytest.mark.parametrize("shading", [True, False])
def test_end_to_end_reconstruction(shading):
    """optimize_shape's loop body (scripts/main.py:172-208) for 300 steps with one remesh at step 150: source icosphere(6), target a
    bumpy icosphere(12), 8 views at 64 x 64, L1 image loss, lambda = 10."""
    from largesteps import synthetic
    from largesteps.geometry import compute_matrix
    from largesteps.meshops import average_edge_length, remove_duplicates
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    from largesteps.optimize import AdamUniform
    from largesteps.parameterize import to_differential, from_differential
    from largesteps.remesh import remesh_botsch
    renderer, ref, tvt, tft = _body_parts(shading)
    v, f = synthetic.icosphere(6)
    v_src, f_src = torch.from_numpy(0.8 * v).to(DEV), torch.from_numpy(f).to(DEV)
    v_u, f_u, dup = remove_duplicates(v_src, f_src)
    M = compute_matrix(v_u, f_u, lambda_=10.0)
    u = to_differential(M, v_u).clone().requires_grad_(True)
    step_size = 3e-2
    opt = AdamUniform([u], step_size)
    d0 = _surface_distance(v_u, tvt)
    losses = []
    for it in range(300):
        if it == 150:
            with torch.no_grad():
                v_u = from_differential(M, u, 'Cholesky')
                h = average_edge_length(v_u, f_u) * 0.5
                v_src, f_src = remesh_botsch(v_u.contiguous(), f_u.to(torch.int32), 5, h, True)
                v_u, f_u, dup = remove_duplicates(v_src, f_src)
                M = compute_matrix(v_u, f_u, lambda_=10.0)
                u = to_differential(M, v_u).clone().requires_grad_(True)
                step_size *= 0.8
                opt = AdamUniform([u], step_size)
        x = from_differential(M, u, 'Cholesky')
        n = compute_vertex_normals(x, f_u, compute_face_normals(x, f_u))
        loss = (renderer.render(x[dup], n[dup], f_src) - ref).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        x = from_differential(M, u, 'Cholesky')
    d1 = _surface_distance(x, tvt)
    ratio = losses[0] / np.mean(losses[-10:])
    print(f"shading={shading}: loss {losses[0]:.5f} -> {np.mean(losses[-10:]):.5f} (x{ratio:.1f}), distance {d0:.4f} -> {d1:.4f}")
    # measured on the MI355X (same seeds): loss x151.5 with shading, x82.1 for silhouettes; mean distance from the vertices to the
    # nearest target vertex 0.192 -> 0.038 / 0.040 (the target's own vertex spacing is ~0.05, so ~0.025 is the floor of this measure)
    assert ratio >= 20.0
    assert d1 <= 0.06
