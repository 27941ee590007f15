"""
largesteps.render on the device at production shapes, against tests/render_statement_fast.py (the vectorised statement, itself proven
equal to tests/render_statement.py by tests/test_render_statement_cpu.py).

- rasterize: triangle ids exact, u, v, z/w within 1 ulp, on the bench's 70k noisy sphere (256^2 x 8 views, 512^2 x 2), a full-screen
  quad at 4096^2 (65 536 tiles a triangle: the cooperative path's tile walk and its binary search), 1 x 4096 and 4096 x 1 strips, a
  17 x 33 frame, random soups crossing w = 0 and duplicated faces (exact depth ties: the lower id).
- ls_raster_pixel_order on fabricated frames: exact against a stable argsort and searchsorted, at B F on both sides of each switch of
  the number of radix passes (256, 65 536, 2^24) and at B H W on both sides of each chunk-size switch of radix.h (2^21, 2^22).
- the backwards, element by element: |dev - ref| <= (depth + slack) 2^-24 abs, abs = the sum of the absolute values of the element's
  terms. depth is the length of the kernel's fp32 summation chain through k_rs_seg_sum (a face of m <= 64 pixels: m terms in order;
  longer: ceil(m / 64) a lane, then 6 butterfly levels) and the per-vertex pass (the vertex's corners; B times that when one attribute
  batch is shared); slack counts the roundings inside a term (see each check). No max-normalised tolerance.
"""
import ctypes
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

import render_statement_fast as rf  # noqa: E402
from render_scenes import bench_views, look_at, random_soup, scene, sphere70k  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = rf.U
RATIOS = {}          # largest |dev - ref| / bound seen per check (printed with -s)


def to_dev(pos, f, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(pos)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV, dtype)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def within(name, dev, ref, bnd):
    """every element within its bound; records the largest ratio"""
    err = np.abs(np.asarray(dev, np.float64) - ref)
    ratio = err / np.maximum(bnd, 1e-300)
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    print(f"{name}: max |dev - ref| / bound = {worst:.3g}")
    bad = np.argwhere(err > bnd)
    assert len(bad) == 0, f"{name}: {len(bad)} elements beyond the bound, first {bad[:3].tolist()}, ratio {worst:.3g}"


def check_rast(got, ref, what):
    assert np.array_equal(got[..., 3], ref[..., 3]), f"{what}: ids differ at {np.argwhere(got[..., 3] != ref[..., 3])[:5].tolist()}"
    assert ulps(got[..., :3], ref[..., :3]).max(initial=0) <= 1, f"{what}: u, v, z/w beyond 1 ulp"


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def quad(H, W):
    pos = np.array([[[-1, -1, 0.5, 1], [1, -1, 0.5, 1], [1, 1, 0.5, 1], [-1, 1, 0.5, 1]]], np.float32)
    return pos, np.array([[0, 1, 2], [0, 2, 3]]), H, W


def duplicated(seed=0):
    """icosphere(4) from three views with every face twice, in shuffled order"""
    from largesteps import synthetic
    from render_scenes import clip
    v, f = synthetic.icosphere(4)
    views = [look_at((0.3, 0.4, -3.0)), look_at((2.5, 1.0, 1.0)), look_at((-1.0, -2.0, 2.0))]
    f2 = np.concatenate([f, f])[np.random.default_rng(seed).permutation(2 * len(f))]
    return clip(v, views), f2, 40, 56


def big_soup():
    return random_soup(4, n=400, B=4, H=64, W=96)


SCALE = {
    "sphere512x2": lambda: sphere70k(2, 512),
    "quad4096": lambda: quad(4096, 4096),
    "strip1x4096": lambda: sphere70k(1, 256)[:2] + (1, 4096),
    "strip4096x1": lambda: sphere70k(1, 256)[:2] + (4096, 1),
    "sphere17x33": lambda: scene("sphere")[:2] + (17, 33),
    "soup": big_soup,
    "duplicates": duplicated,
}


@pytest.fixture(scope="module")
def sphere256():
    """the 70k sphere at 256^2 x 8 views, rasterized on the device and by the statement (shared by the tests below)"""
    import largesteps.render as dr
    pos, f, H, W = sphere70k(8, 256)
    tp, tf = to_dev(pos, f)
    rast = dr.rasterize(None, tp, tf, (H, W))[0].cpu().numpy()
    return pos, f, H, W, rast, rf.rasterize(pos, f, H, W)


def test_rasterize_sphere70k_8_views(sphere256):
    pos, f, H, W, got, ref = sphere256
    check_rast(got, ref, "sphere 256 x 8")
    assert 0.3 < (ref[..., 3] > 0).mean() < 0.9


@pytest.mark.parametrize("name", list(SCALE))
def test_rasterize_at_scale(name):
    import largesteps.render as dr
    pos, f, H, W = SCALE[name]()
    tp, tf = to_dev(pos, f)
    got = dr.rasterize(None, tp, tf, (H, W))[0].cpu().numpy()
    ref = rf.rasterize(pos, f, H, W)
    check_rast(got, ref, name)
    cov = (ref[..., 3] > 0).mean()
    assert cov == 1.0 if name == "quad4096" else cov > 0.0
    if name == "soup":
        assert (pos[..., 3] <= 0).mean() > 0.15
    if name == "duplicates":                      # each covered pixel shows the lower id of its pair of identical faces
        ids = ref[..., 3].astype(np.int64)[ref[..., 3] > 0] - 1
        key = np.sort(f, 1)
        _, first = np.unique(key, axis=0, return_index=True)
        _, inv = np.unique(key, axis=0, return_inverse=True)
        assert np.all(ids == first[inv.ravel()][ids]) and len(ids) > 1000


# ---- pixel order ---------------------------------------------------------------------------------------------------------------------
def _fabricated(B, F, H, W, seed):
    rng = np.random.default_rng(seed)
    N = B * H * W
    ids = rng.integers(1, F + 1, N).astype(np.float64)
    kind = rng.random(N)
    ids[kind < 0.2] = 0.0                                                       # background
    ids[(kind >= 0.2) & (kind < 0.23)] = F + 1 + rng.integers(0, 1000, int(((kind >= 0.2) & (kind < 0.23)).sum()))   # out of range
    ids[(kind >= 0.23) & (kind < 0.25)] = -2.0
    frac = (kind >= 0.25) & (kind < 0.27)
    ids[frac] += 0.5                                                            # rs_id truncates
    ids[:4] = [1, F, 0, F + 1]
    rast = rng.standard_normal((N, 4)).astype(np.float32)
    rast[:, 3] = ids.astype(np.float32)
    r = rast[:, 3]
    valid = (r >= 1.0) & (r <= np.float32(F))
    key = np.where(valid, (np.arange(N) // (H * W)) * F + np.floor(r).astype(np.int64) - 1, B * F)
    return rast.reshape(B, H, W, 4), key


PIXEL_ORDER = [(1, 255, 32, 48), (1, 256, 32, 48), (3, 21845, 64, 64), (2, 32768, 64, 64), (1, (1 << 24) - 1, 64, 64),
               (2, (1 << 23) + 1, 64, 64), (8, 70000, 512, 512), (1, 300, 1025, 2048), (2, 70000, 1024, 2048), (1, 70000, 2049, 2048)]


@pytest.mark.parametrize("B,F,H,W", PIXEL_ORDER)
def test_pixel_order_matches_a_stable_argsort(B, F, H, W):
    from largesteps import _native
    rast, key = _fabricated(B, F, H, W, seed=B * 7 + F % 97)
    N, nk = B * H * W, B * F
    t = torch.from_numpy(rast).to(DEV)
    order = torch.empty(N, dtype=torch.int32, device=DEV)
    seg = torch.empty(nk + 1, dtype=torch.int32, device=DEV)
    n = ctypes.c_size_t(0)
    _native.check(_native.lib().ls_raster_workspace_bytes(B, F, H, W, 0, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    _native.check(_native.lib().ls_raster_pixel_order(_native.ptr(t), B, F, H, W, _native.ptr(order), _native.ptr(seg), _native.ptr(ws),
                                                      ws.numel(), DEV.index, _native.stream_of(DEV)))
    ref = np.argsort(key, kind="stable")
    got = order.cpu().numpy()
    assert np.array_equal(got, ref), f"order differs at {np.nonzero(got != ref)[0][:5].tolist()}"
    assert np.array_equal(seg.cpu().numpy(), np.searchsorted(key[ref], np.arange(nk + 1), side="left"))


# ---- backwards -----------------------------------------------------------------------------------------------------------------------
def _weights(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def check_rasterize_backward(name, pos, f, rast, g_rast, dev_grad, plus=None):
    """rasterize's position gradient. A term (a face row entry of one pixel) is formed in fp64 and rounded once to fp32; the face row
    sums its terms in the kernel's order, the per-vertex pass the vertex's rows: |err| <= (depth + 2) u abs (the 2: the term's
    rounding and second-order terms). plus = (ref, abs, bound) of another gradient that autograd adds to the same tensor (one more
    rounding of both)."""
    B, V = pos.shape[0], pos.shape[1]
    gp, ab = rf.rasterize_backward(pos, f, rast, g_rast)
    depth = rf.vertex_depth(rf.seg_depth(rf.face_pixels(rast, len(f))), f, V)[..., None]
    bnd = rf.bound(depth, ab, 2)
    if plus is not None:
        gp = gp + plus[0]
        bnd = bnd + plus[2] + U * (ab + plus[1])
    within(name, dev_grad, gp, bnd)
    assert np.all(dev_grad[..., 2] == 0)
    return gp


def check_interpolate_backward(name, attr, f, rast, g, dev_ga, dev_gr=None):
    """interpolate's attribute gradient: terms u g, v g and w g with w = (1 - u) - v formed in fp32 (abs of the third: |g| (|1 - u| +
    |v| + |w|), which covers w's two roundings), one rounding per product, then the face row and the per-vertex chain: (depth + 2) u
    abs. grad_rast: sum over the C channels of g_c (a_ic - a_2c), a rounding per difference and product and C - 1 additions: (C + 2) u
    abs."""
    a3 = attr if attr.ndim == 3 else attr[None]
    Ba, V, C = a3.shape
    ga, gr, aga, agr = rf.interpolate_backward(attr, rast, f, g)
    dface = rf.seg_depth(rf.face_pixels(rast, len(f)))
    depth = rf.vertex_depth(dface, f, V, batches_summed=Ba == 1).reshape(attr.shape[:-1] + (1,))
    within(name + " attr", dev_ga, ga, rf.bound(depth, aga, 2))
    k = np.bincount(np.asarray(f).ravel(), minlength=V)
    unref = np.nonzero(k == 0)[0]
    assert np.all(np.take(dev_ga, unref, axis=-2) == 0)
    if dev_gr is not None:
        within(name + " rast", dev_gr[..., :2], gr[..., :2], (C + 2) * U * agr[..., :2])
        assert np.all(dev_gr[..., 2:] == 0)
    return ga, gr


def check_antialias_backward(name, color, rast, pos, f, g, boost, dev_gc, dev_gp=None):
    """antialias. grad_color: the pixel's g and a fac g term per pair, fac = |alpha - 1/2| rounded to fp32, one product rounding,
    the additions in pair order: (terms + 2) u abs. grad_pos: a term is dl dA_q, dl = boost sum_c g_c (c_s - c_r) in fp32 (a rounding
    per difference and product, C - 1 additions: C + 1), the boost and the dA product (2 more): (depth + C + 5) u abs, depth = the
    face row's chain of (pixel, pair) terms and the vertex's corners. Returns (ref grad_pos, its abs, its bound)."""
    B, V, C = pos.shape[0], pos.shape[1], color.shape[-1]
    gc, gp, agc, agp, ngc, nterm = rf.antialias_backward(color, rast, pos, f, g, boost)
    within(name + " color", dev_gc, gc, rf.bound(ngc[..., None], agc, 2))
    depth = rf.vertex_depth(rf.seg_depth(rf.face_pixels(rast, len(f)), terms=nterm), f, V)[..., None]
    bnd = rf.bound(depth, agp, C + 5)
    if dev_gp is not None:
        within(name + " pos", dev_gp, gp, bnd)
    return gp, agp, bnd


def _pad_unreferenced(pos, n=5):
    """n extra vertices no face uses (their gradients must be exactly 0)"""
    extra = np.repeat(pos[:, :1], n, axis=1) + np.float32(0.01)
    return np.concatenate([pos, extra], axis=1)


def test_rasterize_interpolate_antialias_backward_sphere70k(sphere256):
    """the whole primitive chain with pos_gradient_boost 2.5 on the 70k sphere, 256^2 x 8 views: every backward checked with the
    device's own incoming gradient, so each bound is that of one kernel chain"""
    import largesteps.render as dr
    pos, f, H, W, _, ref = sphere256
    pos = _pad_unreferenced(pos)
    B, V = pos.shape[0], pos.shape[1]
    attr = np.random.default_rng(2).uniform(0, 1, (1, V, 3)).astype(np.float32)
    tp, tf = to_dev(pos, f)
    tp.requires_grad_(True)
    ta = torch.from_numpy(attr).to(DEV).requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    rast.retain_grad()
    col = dr.interpolate(ta, rast, tf)[0]
    col.retain_grad()
    out = dr.antialias(col, rast, tp, tf, pos_gradient_boost=2.5)
    G = _weights(out.shape, 3)
    (out * torch.from_numpy(G).to(DEV)).sum().backward()
    r, c = rast.detach().cpu().numpy(), col.detach().cpu().numpy()
    check_rast(r, ref, "sphere 256 x 8 (padded)")
    assert np.array_equal(c, rf.interpolate(attr, r, f))
    assert np.array_equal(out.detach().cpu().numpy(), rf.antialias(c, r, pos, f))
    gp_aa, agp_aa, b_aa = check_antialias_backward("sphere aa", c, r, pos, f, G, 2.5, col.grad.cpu().numpy())
    check_interpolate_backward("sphere interp", attr, f, r, col.grad.cpu().numpy(), ta.grad.cpu().numpy(), rast.grad.cpu().numpy())
    dev_gp = tp.grad.cpu().numpy()
    check_rasterize_backward("sphere rast+aa pos", pos, f, r, rast.grad.cpu().numpy(), dev_gp, plus=(gp_aa, agp_aa, b_aa))
    assert np.all(dev_gp[:, -5:] == 0)


@pytest.mark.parametrize("C,shape", [(1, "V"), (4, "1V"), (7, "BV"), (16, "BV"), (3, "V")])
def test_interpolate_channels_and_attribute_batches(sphere256, C, shape):
    import largesteps.render as dr
    pos, f, H, W, r, _ = sphere256
    B, V = pos.shape[0], pos.shape[1]
    a = np.random.default_rng(C).uniform(-1, 1, {"V": (V, C), "1V": (1, V, C), "BV": (B, V, C)}[shape]).astype(np.float32)
    tr = torch.from_numpy(r).to(DEV).requires_grad_(True)
    ta = torch.from_numpy(a).to(DEV).requires_grad_(True)
    tf = torch.from_numpy(f).to(DEV)
    out = dr.interpolate(ta, tr, tf)[0]
    assert np.array_equal(out.detach().cpu().numpy(), rf.interpolate(a, r, f))
    g = _weights(out.shape, 10 + C)
    (out * torch.from_numpy(g).to(DEV)).sum().backward()
    assert ta.grad.shape == ta.shape
    check_interpolate_backward(f"C={C} {shape}", a, f, r, g, ta.grad.cpu().numpy(), tr.grad.cpu().numpy())


def test_quad_4096_long_segments():
    """two faces of 8M pixels each: k_rs_seg_sum's wave path over 131 072 pixels a lane, for rasterize and interpolate"""
    import largesteps.render as dr
    pos, f, H, W = quad(4096, 4096)
    pos = pos.copy()
    pos[0, :, 3] = [1.0, 1.25, 0.8, 1.1]                                       # perspective: u, v vary non-linearly
    tp, tf = to_dev(pos, f)
    tp.requires_grad_(True)
    a = np.random.default_rng(1).uniform(-1, 1, (4, 2)).astype(np.float32)
    ta = torch.from_numpy(a).to(DEV).requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    rast.retain_grad()
    out = dr.interpolate(ta, rast, tf)[0]
    # weights of one sign: the attribute gradient's terms then do not cancel, so a lost share of a face's millions of terms shows
    # against the wave path's bound of (ceil(m / 64) + 6 + 2) 2^-24 sum|terms| (with zero-mean weights the sum of half the terms is only
    # O(sqrt(m)) of sum|terms| and would pass it)
    g = np.random.default_rng(4).uniform(0.5, 1.5, out.shape).astype(np.float32)
    (out * torch.from_numpy(g).to(DEV)).sum().backward()
    r = rast.detach().cpu().numpy()
    check_rast(r, rf.rasterize(pos, f, H, W), "quad 4096")
    assert rf.face_pixels(r, 2).min() > 4_000_000
    check_interpolate_backward("quad interp", a, f, r, g, ta.grad.cpu().numpy(), rast.grad.cpu().numpy())
    check_rasterize_backward("quad rast", pos, f, r, rast.grad.cpu().numpy(), tp.grad.cpu().numpy())


# ---- the renderer --------------------------------------------------------------------------------------------------------------------
def _renderer(B, res):
    from largesteps.render import NVDRenderer
    th = np.linspace(0, np.pi, 32)[:, None]
    ph = np.linspace(0, 2 * np.pi, 64)[None, :]
    e = np.stack([0.6 + 0.4 * np.cos(th) + 0 * ph, 0.5 + 0.3 * np.sin(th) * np.cos(ph), 0.4 + 0.3 * np.cos(2 * th) + 0 * ph,
                  np.ones((32, 64))], -1).astype(np.float32)
    params = {"res_x": res, "res_y": res, "fov": 45.0, "near_clip": 0.1, "far_clip": 100.0, "envmap_scale": 1.0,
              "view_mats": [torch.from_numpy(M).float().to(DEV) for M in bench_views(B)], "envmap": torch.from_numpy(e).to(DEV)}
    return NVDRenderer(params, shading=True, boost=3.0)


def _render_pass(R, v, n, tf, G):
    """NVDRenderer.render's body with its intermediates kept (the test checks it is bitwise the same image as render())"""
    import largesteps.render as dr
    vp = v.clone().requires_grad_(True)
    np_ = n.clone().requires_grad_(True)
    v_ndc = torch.matmul(torch.nn.functional.pad(vp, (0, 1), 'constant', 1.0), R.mvps.transpose(1, 2))
    v_ndc.retain_grad()
    rast = dr.rasterize(R.glctx, v_ndc, tf, R.res)[0]
    rast.retain_grad()
    light = R.sh.eval(np_).contiguous()[None, ...]
    light.retain_grad()
    li = dr.interpolate(light, rast, tf)[0]
    li.retain_grad()
    col = torch.cat((li / np.pi, torch.ones((*li.shape[:-1], 1), device=DEV)), dim=-1)
    shaded = torch.where(rast[..., -1:] != 0, col, R.bgs)
    shaded.retain_grad()
    img = dr.antialias(shaded, rast, v_ndc, tf, pos_gradient_boost=R.boost)
    (img * G).sum().backward()
    return {k: t.detach().cpu().numpy() for k, t in dict(img=img, v_ndc=v_ndc, rast=rast, light=light, shaded=shaded,
                                                       g_vndc=v_ndc.grad, g_rast=rast.grad, g_light=light.grad, g_li=li.grad, g_shaded=shaded.grad,
                                                       g_v=vp.grad, g_n=np_.grad, li=li).items()}


def test_nvdrenderer_render_70k_8_views():
    """NVDRenderer.render forward and backward with shading on the 70k sphere at 256^2 x 8: the image against the composed statement
    (2e-6), each kernel's backward under its per-element bound, v.grad and n.grad with those bounds carried through the (fp32 torch)
    projection and spherical-harmonic products, and two runs bitwise identical"""
    from largesteps import synthetic
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    tv, tf = torch.from_numpy(v.astype(np.float32)).to(DEV), torch.from_numpy(np.asarray(f, np.int64)).to(DEV)
    tn = compute_vertex_normals(tv, tf, compute_face_normals(tv, tf))
    R = _renderer(8, 256)
    G = torch.from_numpy(_weights((8, 256, 256, 4), 12)).to(DEV)
    a = _render_pass(R, tv, tn, tf, G)
    b = _render_pass(R, tv, tn, tf, G)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["img"], R.render(tv, tn, tf).detach().cpu().numpy())
    pos, r, Gn = a["v_ndc"], a["rast"], G.cpu().numpy()
    f = np.asarray(f, np.int64)
    check_rast(r, rf.rasterize(pos, f, 256, 256), "renderer")
    li = rf.interpolate(a["light"], r, f)
    assert np.array_equal(li, a["li"])
    assert np.abs(a["img"] - rf.antialias(a["shaded"], r, pos, f)).max() <= 2e-6
    gp_aa, agp_aa, b_aa = check_antialias_backward("renderer aa", a["shaded"], r, pos, f, Gn, 3.0, a["g_shaded"])
    ga, _ = check_interpolate_backward("renderer interp", a["light"], f, r, a["g_li"], a["g_light"])
    gp = check_rasterize_backward("renderer pos", pos, f, r, a["g_rast"], a["g_vndc"], plus=(gp_aa, agp_aa, b_aa))
    # carried through: v_ndc = [v, 1] M_b^T, so v.grad = sum_b g_b M_b[:, :3]. The device's g_b is within bnd_b of gp_b; torch's fp32
    # product and the sum over the 8 views add at most (4 + 8 + 2) roundings of sum_b |g_b| |M_b|.
    M = R.mvps.double().cpu().numpy()
    V = pos.shape[1]
    dev_g = a["g_vndc"].astype(np.float64)
    err_prop = np.abs(dev_g - gp)                             # already shown to lie within the per-element bound
    ref_v = np.einsum("bvi,bij->vj", gp, M[:, :, :3])
    bound_v = np.einsum("bvi,bij->vj", err_prop, np.abs(M[:, :, :3])) + 14 * U * np.einsum("bvi,bij->vj", np.abs(dev_g), np.abs(M[:, :, :3]))
    within("renderer v.grad", a["g_v"], ref_v, bound_v * (1 + 1e-6) + 1e-30)
    # n.grad: light_c = nh^T M_c nh, d/dn = ((M_c + M_c^T) nh)[:3]; torch's fp32 products of 4-term sums: 12 roundings of |M| |nh| |g|
    Msh = R.sh.M.double().cpu().numpy()
    nh = np.concatenate([tn.double().cpu().numpy(), np.ones((V, 1))], 1)
    J = np.einsum("cij,vj->vci", Msh + Msh.transpose(0, 2, 1), nh)[..., :3]
    Ja = np.einsum("cij,vj->vci", np.abs(Msh) + np.abs(Msh.transpose(0, 2, 1)), np.abs(nh))[..., :3]
    dev_ga = a["g_light"][0].astype(np.float64)
    ref_n = np.einsum("vc,vci->vi", ga[0], J)
    bound_n = np.einsum("vc,vci->vi", np.abs(dev_ga - ga[0]), Ja) + 12 * U * np.einsum("vc,vci->vi", np.abs(dev_ga), Ja)
    within("renderer n.grad", a["g_n"], ref_n, bound_n * (1 + 1e-6) + 1e-30)


# ---- small edges ---------------------------------------------------------------------------------------------------------------------
def test_no_faces():
    import largesteps.render as dr
    pos, _, H, W = scene("sphere")
    tp = torch.from_numpy(pos).to(DEV).requires_grad_(True)
    tf = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    ta = torch.rand((pos.shape[1], 3), device=DEV).requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    col = dr.interpolate(ta, rast, tf)[0]
    out = dr.antialias(col + 1.0, rast, tp, tf)
    (out * torch.rand_like(out)).sum().backward()
    assert torch.count_nonzero(rast) == 0 and torch.count_nonzero(col) == 0
    assert torch.equal(out, torch.ones_like(out))
    assert torch.count_nonzero(tp.grad) == 0 and torch.count_nonzero(ta.grad) == 0


@pytest.mark.parametrize("H,W", [(1, 64), (64, 1), (1, 1)])
def test_single_row_and_column_through_antialias(H, W):
    import largesteps.render as dr
    pos, f, _, _ = scene("sphere_b3")
    pos = pos * np.array([4, 4, 1, 1], np.float32)                           # large on screen: the one row / column crosses it
    B, V = pos.shape[0], pos.shape[1]
    tp, tf = to_dev(pos, f)
    tp.requires_grad_(True)
    attr = np.random.default_rng(3).uniform(0, 1, (V, 3)).astype(np.float32)
    ta = torch.from_numpy(attr).to(DEV).requires_grad_(True)
    rast = dr.rasterize(None, tp, tf, (H, W))[0]
    rast.retain_grad()
    col = dr.interpolate(ta, rast, tf)[0]
    col.retain_grad()
    out = dr.antialias(col, rast, tp, tf, pos_gradient_boost=1.5)
    G = _weights(out.shape, 5)
    (out * torch.from_numpy(G).to(DEV)).sum().backward()
    r, c = rast.detach().cpu().numpy(), col.detach().cpu().numpy()
    check_rast(r, rf.rasterize(pos, f, H, W), f"{H}x{W}")
    assert np.array_equal(out.detach().cpu().numpy(), rf.antialias(c, r, pos, f))
    plus = check_antialias_backward(f"{H}x{W} aa", c, r, pos, f, G, 1.5, col.grad.cpu().numpy())
    check_interpolate_backward(f"{H}x{W} interp", attr, f, r, col.grad.cpu().numpy(), ta.grad.cpu().numpy(), rast.grad.cpu().numpy())
    check_rasterize_backward(f"{H}x{W} pos", pos, f, r, rast.grad.cpu().numpy(), tp.grad.cpu().numpy(), plus=plus)
    assert (r[..., 3] > 0).any()
    if H * W == 1:                                                            # no pair at all
        assert np.array_equal(out.detach().cpu().numpy(), c)


def test_noncontiguous_int64_faces_and_float64_positions():
    import largesteps.render as dr
    pos, f, H, W = scene("sphere_b3")
    attr = np.random.default_rng(4).uniform(0, 1, (pos.shape[1], 3)).astype(np.float32)

    def run(tp, tf):
        tp = tp.requires_grad_(True)
        ta = torch.from_numpy(attr).to(DEV).requires_grad_(True)
        rast = dr.rasterize(None, tp, tf, (H, W))[0]
        col = dr.interpolate(ta, rast, tf)[0]
        out = dr.antialias(col, rast, tp, tf)
        (out * torch.from_numpy(_weights(out.shape, 8)).to(DEV)).sum().backward()
        return [t.detach().float().cpu().numpy() for t in (rast, col, out, tp.grad, ta.grad)]

    tp, tf = to_dev(pos, f)
    a = run(tp, tf.to(torch.int32))
    wide = torch.cat([tf, tf + 1], 1)[:, :3]
    assert not wide.is_contiguous() and wide.dtype == torch.int64
    p64 = torch.from_numpy(pos.astype(np.float64)).to(DEV)
    b = run(p64, wide)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
