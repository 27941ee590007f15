"""
largesteps.render without a device: the numpy statement (tests/render_statement.py) against the reference's own numbers
(tests/golden/reference_render.npz, tests/golden/make_golden_render.py), its watertightness, antialias continuity and backward
against finite differences, and the public surface against the reference's nvdiffrast / NVDRenderer call sites.
"""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import render_statement as rs  # noqa: E402
from render_scenes import grid_mesh as _grid_mesh  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "reference_render.npz"))


# ---- public surface ----------------------------------------------------------------------------------------------------------------
def test_api_surface_matches_the_reference_call_sites():
    import largesteps.render as dr
    assert list(inspect.signature(dr.rasterize).parameters) == ["glctx", "pos", "tri", "resolution", "ranges", "grad_db"]
    assert list(inspect.signature(dr.interpolate).parameters) == ["attr", "rast", "tri", "rast_db", "diff_attrs"]
    assert list(inspect.signature(dr.antialias).parameters) == ["color", "rast", "pos", "tri", "topology_hash", "pos_gradient_boost"]
    assert list(inspect.signature(dr.texture).parameters)[:2] == ["tex", "uv"]
    assert dr.RasterizeGLContext is dr.RasterizeContext and dr.RasterizeCudaContext is dr.RasterizeContext
    dr.RasterizeGLContext()
    assert list(inspect.signature(dr.NVDRenderer).parameters) == ["scene_params", "shading", "boost"]
    assert inspect.signature(dr.NVDRenderer).parameters["shading"].default is True
    assert list(inspect.signature(dr.NVDRenderer.render).parameters) == ["self", "v", "n", "f"]
    assert list(inspect.signature(dr.persp_proj).parameters)[:4] == ["fov_x", "ar", "near", "far"]
    with pytest.raises(NotImplementedError):
        dr.rasterize(None, torch.zeros(4, 4), torch.zeros((1, 3), dtype=torch.int32), (8, 8), ranges=torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):           # no CPU path
        dr.rasterize(None, torch.zeros(1, 3, 4), torch.zeros((1, 3), dtype=torch.int32), (8, 8))
    with pytest.raises(ValueError):
        dr.rasterize(None, torch.zeros(1, 3, 4), torch.zeros((1, 3), dtype=torch.int32), (8, 5000))


def test_native_entry_points_are_bound():
    from largesteps import _native
    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_raster_")]
    assert sorted(names) == sorted(["ls_raster_workspace_bytes", "ls_raster_forward", "ls_raster_pixel_order", "ls_raster_backward",
                                    "ls_raster_interpolate", "ls_raster_interpolate_backward", "ls_raster_adjacency_workspace_bytes",
                                    "ls_raster_adjacency", "ls_raster_antialias", "ls_raster_antialias_backward"])


def test_no_float_atomics_in_the_rasterizer():
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "raster.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src


# ---- the renderer's non-rasterizer parts against the reference's numbers -------------------------------------------------------------
def test_spherical_harmonics_and_projection_match_the_reference(golden):
    from largesteps.render import SphericalHarmonics, persp_proj
    sh = SphericalHarmonics(torch.from_numpy(golden["sh_envmap"]))
    np.testing.assert_allclose(sh.M.numpy(), golden["sh_M"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sh.eval(torch.from_numpy(golden["sh_normals"])).numpy(), golden["sh_eval"], rtol=1e-5, atol=1e-6)
    for a, P in zip(golden["proj_args"], golden["proj"]):
        np.testing.assert_array_equal(persp_proj(*a).numpy(), P)


def test_background_coordinates_match_the_reference(golden):
    from largesteps.render import NVDRenderer
    H, W = (int(x) for x in golden["bg_res"])
    r = NVDRenderer.__new__(NVDRenderer)
    r.res, r.fov_x = (H, W), golden["bg_fov"].item()
    r.view_mats = torch.from_numpy(golden["bg_view_mats"])
    np.testing.assert_allclose(r.background_uvs().numpy(), golden["bg_uvs"], rtol=0, atol=2e-6)


def test_texture_is_bilinear_with_texel_centres_and_wrap():
    from largesteps.render import texture
    tex = torch.arange(12, dtype=torch.float32).reshape(1, 3, 4, 1)
    uv = torch.tensor([[[[0.125, 1 / 6], [0.25, 1 / 6], [0.0, 1 / 6]]]])
    out = texture(tex, uv)[0, 0, :, 0].numpy()
    np.testing.assert_allclose(out, [0.0, 0.5, 1.5], atol=1e-6)   # centre of texel 0; halfway to texel 1; halfway between 3 and 0 (wrap)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def _coverage_count(pos, f, H, W):
    py, px = np.meshgrid(rs.centres(H), rs.centres(W), indexing="ij")
    cnt = np.zeros((H, W), dtype=np.int64)
    for t in f:
        cnt += rs.cover(pos[0, t], px, py)[0]
    return cnt


def test_watertight_on_pixel_centres():
    """vertices exactly on pixel centres (W = H = 16: the centres are dyadic): every edge and vertex runs through centres"""
    W = H = 16
    c = rs.centres(W)
    step = c[1] - c[0]
    n = W // 2 + 3
    pos, f = _grid_mesh(n, 0, 0, coords=c[0] + step * (2 * np.arange(n) - 2))
    assert np.isin(pos[0, :, 0], c.astype(np.float32)).sum() > 0
    assert np.all(_coverage_count(pos, f, H, W) == 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_watertight_on_random_tessellations(seed):
    pos, f = _grid_mesh(9, -1.25, 1.25, jitter=0.12, seed=seed, wscale=seed > 0)
    assert np.all(_coverage_count(pos, f, 24, 32) == 1)


def test_zero_area_triangles_cover_nothing():
    pos = np.array([[[-1, -1, 0, 1], [1, 1, 0, 1], [0, 0, 0, 1]]], np.float32)
    assert not _coverage_count(pos, np.array([[0, 1, 2]]), 8, 8).any()


def test_near_plane_matches_homogeneous_clipping():
    """triangles through the near plane and through w = 0: the edge-function rule with z/w in [-1, 1] against Sutherland-Hodgman
    clipping in homogeneous space, at every pixel centre not within 1e-6 of a clipped polygon's edge"""
    rng = np.random.default_rng(3)
    H, W = 24, 24
    py, px = np.meshgrid(rs.centres(H), rs.centres(W), indexing="ij")
    checked = 0
    for _ in range(40):
        q = np.concatenate([rng.uniform(-2, 2, (3, 2)), rng.uniform(-1.5, 2.5, (3, 1))], 1)      # (x, y, view depth)
        zv = q[:, 2]
        near, far = 0.5, 10.0
        P = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, (far + near) / (far - near), -2 * far * near / (far - near)], [0, 0, 1, 0]])
        clipq = (np.concatenate([q[:, :2], zv[:, None], np.ones((3, 1))], 1) @ P.T).astype(np.float32)
        m_edge = rs.cover(clipq, px, py)[0]
        m_clip = rs.clip_cover(clipq, px, py)
        eps_pos = rs.clip_cover(clipq, px + 1e-6, py) & rs.clip_cover(clipq, px - 1e-6, py) & rs.clip_cover(clipq, px, py + 1e-6) & \
            rs.clip_cover(clipq, px, py - 1e-6)
        eps_neg = ~(rs.clip_cover(clipq, px + 1e-6, py) | rs.clip_cover(clipq, px - 1e-6, py) | rs.clip_cover(clipq, px, py + 1e-6) |
                    rs.clip_cover(clipq, px, py - 1e-6))
        firm = eps_pos | eps_neg
        assert np.array_equal(m_edge[firm], m_clip[firm])
        checked += int(m_clip.any())
    assert checked >= 10


def _tri_scene(dx):
    """one triangle over the background, vertex 0 moved along x by dx NDC units"""
    pos = np.array([[[-0.7 + dx, -0.6, 0.2, 1.0], [0.6, -0.35, 0.2, 1.0], [0.05, 0.7, 0.2, 1.0]]], np.float32)
    return pos, np.array([[0, 1, 2]])


def test_antialias_is_continuous_in_the_vertex_positions():
    """a vertex swept across pixel centres in steps of 3/1000 pixel: the raw coverage jumps by 1 where a silhouette edge crosses a centre,
    the antialiased image by O(step). Within 1.5 pixels of the moving vertex itself, where two silhouette edges meet and each pair
    sees only one of them, the rule is not continuous; those pixels are left out."""
    H = W = 16
    step = 2.0 / W / 1000
    prev_raw = prev_aa = None
    max_raw = max_aa = 0.0
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for k in range(0, 2400, 3):
        pos, f = _tri_scene(k * step)
        rast = rs.rasterize(pos, f, H, W)
        col = rs.interpolate(np.ones((3, 1), np.float32), rast, f)
        aa = rs.antialias(col, rast, pos, f)
        vx, vy = (pos[0, 0, 0] + 1) * W / 2, (pos[0, 0, 1] + 1) * H / 2
        far = np.hypot(xs - vx, ys - vy) > 1.5
        if prev_raw is not None:
            max_raw = max(max_raw, np.abs(col - prev_raw)[0, ..., 0][far].max())
            max_aa = max(max_aa, np.abs(aa - prev_aa)[0, ..., 0][far].max())
        prev_raw, prev_aa = col, aa
    assert max_raw == 1.0                 # centres were crossed
    assert max_aa <= 0.01, max_aa


def test_statement_backward_matches_finite_differences():
    from largesteps import synthetic
    v, f = synthetic.icosphere(2)
    vh = np.concatenate([v, np.ones((v.shape[0], 1), np.float32)], 1)
    P = np.array([[1.2, 0, 0, 0], [0, 1.2, 0, 0], [0, 0, 1.02, -0.2], [0, 0, 1, 0]])
    pos = (vh @ P.T + np.array([0.1, -0.05, 3.0, 3.0])).astype(np.float32)[None]
    H, W = 12, 14
    rng = np.random.default_rng(11)
    attr = rng.uniform(0, 1, (v.shape[0], 2)).astype(np.float32)
    rast = rs.rasterize(pos, f, H, W)
    col = rs.interpolate(attr, rast, f)
    g = rng.standard_normal(col.shape)
    # interpolate: linear in attr
    ga, gr = rs.interpolate_backward(attr, rast, f, g)
    d = rng.standard_normal(attr.shape).astype(np.float32)
    fd = ((rs.interpolate(attr + 1e-2 * d, rast, f).astype(np.float64) - rs.interpolate(attr - 1e-2 * d, rast, f)) * g).sum() / 2e-2
    assert abs(fd - (ga * d).sum()) <= 1e-3 * abs(fd)
    # rasterize: u, v on the pixels whose triangle does not change
    gu = rng.standard_normal(rast.shape)
    gu[..., 2:] = 0
    gp = rs.rasterize_backward(pos, f, rast, gu)
    d = rng.standard_normal(pos.shape)
    d[..., 2] = 0
    e = 1e-3
    rp, rm = rs.rasterize((pos + e * d).astype(np.float32), f, H, W), rs.rasterize((pos - e * d).astype(np.float32), f, H, W)
    keep = (rp[..., 3] == rast[..., 3]) & (rm[..., 3] == rast[..., 3]) & (rast[..., 3] > 0)
    gk = gu * keep[..., None]
    fd = ((rp[..., :2].astype(np.float64) - rm[..., :2]) * gk[..., :2]).sum() / (2 * e)
    an = (rs.rasterize_backward(pos, f, rast, gk) * d).sum()
    assert abs(fd - an) <= 1e-2 * abs(an), (fd, an)
    assert np.all(gp[..., 2] == 0)
    # antialias: rast held fixed, colour and positions perturbed
    color = col[..., :1].copy()
    gcol = rng.standard_normal(color.shape)
    gc, gpa = rs.antialias_backward(color, rast, pos, f, gcol)
    dc = rng.standard_normal(color.shape).astype(np.float32)
    fd = ((rs.antialias(color + 1e-2 * dc, rast, pos, f).astype(np.float64) - rs.antialias(color - 1e-2 * dc, rast, pos, f)) * gcol).sum() / 2e-2
    assert abs(fd - (gc * dc).sum()) <= 1e-3 * abs(fd)
    e = 1e-4
    fd = ((rs.antialias(color, rast, (pos + e * d).astype(np.float32), f).astype(np.float64)
           - rs.antialias(color, rast, (pos - e * d).astype(np.float32), f)) * gcol).sum() / (2 * e)
    an = (gpa * d).sum()
    assert abs(an) > 0 and abs(fd - an) <= 2e-2 * abs(an), (fd, an)
