"""
The mipmapped lookup and the pixel differentials of largesteps.render without a device: self-checks of the numpy statement
(tests/mip_statement.py) -- level sizes, means, central finite differences of its own forward --, the flag cap of the device
test's cases (those of tests/texture_cases.py too, with the conditions they were built for), and the public surface (argument checks,
exported symbols, what must not move).
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

import mip_statement as ms  # noqa: E402
import texture_statement as ts  # noqa: E402

MIP_SYMBOLS = ["ls_mip_workspace_bytes", "ls_mip_build", "ls_mip_fold", "ls_mip_pixel_differentials", "ls_mip_interpolate_da", "ls_mip_forward",
               "ls_mip_order", "ls_mip_backward"]


def test_statement_pyramid_sizes_and_means():
    rng = np.random.default_rng(0)

    def sizes(Ht, Wt, max_level=None):
        return [(lv.shape[2], lv.shape[1]) for lv in ms.pyramid(rng.standard_normal((1, Ht, Wt, 2)), max_level)]       # (W, H)

    assert sizes(8, 8) == [(8, 8), (4, 4), (2, 2), (1, 1)]
    assert sizes(2, 4) == [(4, 2), (2, 1), (1, 1)]
    assert sizes(1, 1) == [(1, 1)]
    assert sizes(16, 16, 2) == [(16, 16), (8, 8), (4, 4)]
    for bad in ((6, 5), (6, 8), (12, 12)):                 # 12 -> 6 -> 3: level 2 cannot be halved
        with pytest.raises(ValueError):
            ms.pyramid(np.zeros((1,) + bad + (1,)))
    assert sizes(12, 12, 2) == [(12, 12), (6, 6), (3, 3)]  # ... unless the pyramid stops there
    for lv in ms.pyramid(np.full((2, 8, 4, 3), 0.3, np.float32)):
        assert np.all(lv == np.float32(0.3))
    tex = rng.standard_normal((2, 8, 16, 3)).astype(np.float32)
    for lv in ms.pyramid(tex):
        assert lv.dtype == np.float32
        np.testing.assert_allclose(lv.mean((1, 2)), tex.mean((1, 2)), rtol=0, atol=1e-5)
    # by hand: one 2 x 2 block
    assert ms.pyramid(np.float32([[[[1.0], [2.0]], [[3.0], [6.0]]]]))[1].item() == 3.0


def _inputs(rng, B, H, W, Bt, Ht, Wt, C, Lmax, with_da, with_bias):
    """fp64 inputs away from every kink: uv at least 0.05 of a cell away from the texel centre lines of every level, lod at least 0.15
    away from an integer and inside (0, Lmax). The texture holds multiples of 2^-6, so that the fp32 means of the pyramid are exact and
    the lookup is exactly linear in it."""
    tex = np.round(rng.standard_normal((Bt, Ht, Wt, C)) * 64) / 64
    want = rng.integers(0, max(Lmax, 1), (B, H, W)) + rng.uniform(0.15, 0.85, (B, H, W))
    while True:
        uv = rng.uniform(-0.5, 1.5, (B, H, W, 2))
        ok = np.ones((B, H, W), bool)
        for l in range(Lmax + 1):
            for a, n in ((0, max(Wt >> l, 1)), (1, max(Ht >> l, 1))):
                x = uv[..., a] * n - 0.5
                ok &= np.abs(x - np.round(x)) > 0.05
        if ok.mean() > 0.2:
            break
    uv = np.where(ok[..., None], uv, uv[ok][0])
    da = bias = None
    if with_da:
        d = rng.standard_normal((B, H, W, 4))
        share = want - (rng.uniform(-0.3, 0.3, (B, H, W)) if with_bias else 0.0)
        da = d * np.sqrt(4.0 ** share / ms.footprint(d, Ht, Wt)[0])[..., None]
        if with_bias:
            bias = want - share
    else:
        bias = want
    return tex, uv, da, bias


@pytest.mark.parametrize("boundary", ts.BOUNDARIES)
@pytest.mark.parametrize("mode", ms.MODES)
def test_statement_gradients_match_central_differences(mode, boundary):
    rng = np.random.default_rng(11)
    B, H, W, C = 2, 4, 5, 3
    for Bt, Ht, Wt, with_da, with_bias in ((1, 8, 8, True, True), (2, 2, 4, True, False), (1, 4, 8, False, True)):
        Lmax = ms.last_level(Ht, Wt)
        tex, uv, da, bias = _inputs(rng, B, H, W, Bt, Ht, Wt, C, Lmax, with_da, with_bias)
        g = rng.standard_normal((B, H, W, C))

        def loss(t, c, d, b):
            return float((ms.texture(t, c, d, b, None, mode, boundary, coords=np.float64).out * g).sum())

        r = ms.texture(tex, uv, da, bias, g, mode, boundary, coords=np.float64)
        assert not r.flag.any() and r.finite.all()
        if mode == "linear-mipmap-linear":
            assert r.two.all()
        eps = 1e-6
        for trial in range(2):
            dc = rng.standard_normal(uv.shape)
            fd_c = (loss(tex, uv + eps * dc, da, bias) - loss(tex, uv - eps * dc, da, bias)) / (2 * eps)
            an_c = float((r.grad_uv * dc).sum())
            assert abs(fd_c - an_c) <= 1e-6 * (np.abs(r.grad_uv_abs * np.abs(dc)).sum() + 1.0), ("uv", fd_c, an_c)
            assert abs(an_c) > 1e-3
            dt = np.round(rng.standard_normal(tex.shape) * 4) / 4                 # the pyramid is built in fp32: a step it holds exactly
            h = 2.0 ** -7
            fd_t = (loss(tex + h * dt, uv, da, bias) - loss(tex - h * dt, uv, da, bias)) / (2 * h)          # the lookup is linear in tex
            an_t = float((r.grad_tex * dt).sum())
            assert abs(fd_t - an_t) <= 1e-6 * (np.abs(r.grad_tex_abs * np.abs(dt)).sum() + 1.0), ("tex", fd_t, an_t)
            assert abs(an_t) > 1e-3
            if bias is not None:
                db = rng.standard_normal(bias.shape)
                fd_b = (loss(tex, uv, da, bias + eps * db) - loss(tex, uv, da, bias - eps * db)) / (2 * eps)
                an_b = float((r.grad_bias * db).sum())
                assert abs(fd_b - an_b) <= 1e-6 * (np.abs(r.grad_bias_abs * np.abs(db)).sum() + 1.0), ("bias", fd_b, an_b)
                assert (abs(an_b) > 1e-3) == (mode == "linear-mipmap-linear")
            if da is not None:
                dd = rng.standard_normal(da.shape) * np.abs(da).mean()
                fd_d = (loss(tex, uv, da + eps * dd, bias) - loss(tex, uv, da - eps * dd, bias)) / (2 * eps)
                an_d = float((r.grad_uv_da * dd).sum())
                assert abs(fd_d - an_d) <= 1e-6 * (np.abs(r.grad_uv_da_abs * np.abs(dd)).sum() + 1.0), ("uv_da", fd_d, an_d)
                assert (abs(an_d) > 1e-6) == (mode == "linear-mipmap-linear")


def test_statement_hand_cases():
    tex = (np.indices((8, 8)).sum(0) % 2).astype(np.float32)[None, :, :, None]
    uv = np.random.default_rng(0).uniform(0, 1, (1, 4, 4, 2))
    for lod, want in ((1.0, 0.5), (2.5, 0.5), (7.0, 0.5)):
        assert np.abs(ms.texture(tex, uv, None, np.full((1, 4, 4), lod), None).out - want).max() < 1e-12
    # lod 0 and below is the plain lookup; the two modes agree on integer lods
    plain = ts.texture(tex, uv).out
    for lod in (0.0, -3.0):
        for mode in ms.MODES:
            assert np.array_equal(ms.texture(tex, uv, None, np.full((1, 4, 4), lod), None, mode).out, plain)
    # an isotropic footprint of 4 texels per pixel is lod 2; a zero footprint is level 0
    da = np.zeros((1, 4, 4, 4))
    assert np.array_equal(ms.texture(tex, uv, da, None, None).out, plain)
    da[..., 0] = da[..., 3] = 4.0 / 8
    r = ms.texture(tex, uv, da, None, None)
    assert np.allclose(r.lod, 2.0) and r.flag.all()
    # an anisotropic one takes its major axis
    da[..., 3] = 1.0 / 8
    assert np.allclose(ms.texture(tex, uv, da, None, None).lod, 2.0)
    with pytest.raises(ValueError):
        ms.texture(tex, uv)


def test_the_device_cases_stay_under_the_flag_cap():
    from test_mip_gpu import CASES, COMBOS, case
    for name in CASES:
        tex, uv, da, bias, max_level = case(name)
        for mode, boundary in COMBOS:
            r = ms.texture(tex, uv, da, bias, None, mode, boundary, max_level)
            assert r.flag.mean() <= 0.02, (name, mode, r.flag.mean())
            if name in ("constant_uv", "bias_only"):
                assert not r.flag.any()
            if name == "interpolated":
                assert r.finite.all() and (r.lod[np.abs(uv).sum(-1) > 0] > 0).mean() > 0.5          # the quad is minified: the mip levels are used
        if name == "b1_8x8_c3":
            assert (r.lod < 0).any() and (r.lod > r.Lmax).any()


def test_statement_differentials_match_central_differences_of_the_barycentrics():
    """du/dX of the statement against the barycentrics of the statement's rasterizer one pixel apart, in an affine view (exact there)
    and against the analytic perspective derivative by finite differences of the edge functions elsewhere"""
    import render_statement as rs
    from test_mip_gpu import oblique_quad
    pos, tri, attr, H, W = oblique_quad()
    rast = rs.rasterize(pos, tri, H, W)
    db, mag = ms.pixel_differentials(rast, pos, tri)
    cov = rast[..., 3] > 0
    assert cov.sum() > 50 and not db[~cov].any() and np.all(mag >= np.abs(db) * (1 - 1e-12))
    # central differences of u = a_0 / s in continuous pixel coordinates
    q = pos[0].astype(np.float64)
    for y, x in zip(*np.nonzero(cov[0])):
        p = q[tri[int(rast[0, y, x, 3]) - 1]][:, [0, 1, 3]]
        A = np.stack([np.cross(p[1], p[2]), np.cross(p[2], p[0]), np.cross(p[0], p[1])])

        def uv_at(X, Y):
            e = A @ np.array([(2 * X + 1) / W - 1, (2 * Y + 1) / H - 1, 1.0])
            return e[:2] / e.sum()

        h = 1e-5
        fd = np.concatenate([(uv_at(x + h, y) - uv_at(x - h, y)) / (2 * h), (uv_at(x, y + h) - uv_at(x, y - h)) / (2 * h)])[[0, 2, 1, 3]]
        assert np.abs(fd - db[0, y, x]).max() <= 1e-8 * (1 + mag[0, y, x].max())
    da, _ = ms.attr_da(attr, rast, tri, db)
    assert da.shape == (1, H, W, 4) and da[cov].any() and not da[~cov].any()


def test_argument_checks_need_no_device():
    import largesteps.render as dr
    assert "texture_construct_mip" in dr.__all__ and "pixel_differentials" in dr.__all__
    for bad in ((1, 6, 5, 1), (1, 4, 6, 2)):
        with pytest.raises(ValueError, match="level"):
            dr.texture_construct_mip(torch.zeros(bad))
    with pytest.raises(ValueError, match="level 1 is 3 x 3"):
        dr.texture_construct_mip(torch.zeros(1, 6, 6, 1))
    with pytest.raises(NotImplementedError, match="HIP device"):
        dr.texture_construct_mip(torch.zeros(1, 6, 6, 1), max_mip_level=1)          # sizes are fine: only the device is missing
    with pytest.raises(NotImplementedError):
        dr.texture_construct_mip(torch.zeros(1, 8, 8, 1), cube_mode=True)
    assert dr._mip_last_level(8, 8) == 3 and dr._mip_last_level(2, 4) == 2 and dr._mip_last_level(1, 1) == 0
    assert dr._mip_last_level(16, 16, 2) == 2 and dr._mip_last_level(4, 4, 9) == 2
    uv = torch.zeros(2, 5, 5, 2)
    with pytest.raises(ValueError, match="uv_da or mip_level_bias"):
        dr._check_mip_inputs(uv, None, None)
    with pytest.raises(ValueError, match="uv_da must be"):
        dr._check_mip_inputs(uv, torch.zeros(2, 5, 5, 2), None)
    with pytest.raises(ValueError, match="mip_level_bias must be"):
        dr._check_mip_inputs(uv, None, torch.zeros(2, 5, 5, 1))
    with pytest.raises(TypeError):
        dr._check_mip_inputs(uv, torch.zeros(2, 5, 5, 4).double(), None)
    dr._check_mip_inputs(uv, torch.zeros(2, 5, 5, 4), torch.zeros(2, 5, 5))
    # a mip object is tied to one version of one tensor
    tex = torch.rand(1, 4, 4, 3)
    mip = dr._Mip(tex, 2, None)
    mip.check(tex)
    with pytest.raises(ValueError, match="stale"):
        mip.check(tex.clone())
    tex.add_(1.0)
    with pytest.raises(ValueError, match="stale"):
        mip.check(tex)
    with pytest.raises(ValueError, match="rast_db"):
        dr.interpolate(torch.zeros(3, 2), torch.zeros(1, 4, 4, 4), torch.zeros(1, 3, dtype=torch.int32), diff_attrs='all')


def test_what_must_not_move():
    import largesteps.render as dr
    from largesteps import _native
    tex, uv = torch.rand(1, 4, 4, 3), torch.rand(2, 5, 5, 2)
    for mode in ms.MODES:
        with pytest.raises(NotImplementedError, match="HIP device"):
            dr.texture(tex, uv, filter_mode=mode)
        with pytest.raises(NotImplementedError, match="HIP device"):          # before anything else is checked
            dr.texture(tex.double(), uv[0], filter_mode=mode, boundary_mode="mirror")
    with pytest.raises(NotImplementedError):
        dr.texture(tex, uv, boundary_mode="cube")
    a = dr.texture(tex, uv, uv_da=torch.zeros(1), mip_level_bias=torch.zeros(7), mip=object(), filter_mode="auto", max_mip_level=3)
    assert torch.equal(a, dr.texture(tex, uv, filter_mode="linear"))
    assert _native.lib().ls_version() == 110


def test_native_entry_points_are_exported_and_bound():
    from largesteps import _native
    assert sorted(n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_mip_")) == sorted(MIP_SYMBOLS)
    lib = _native.lib()
    for n in MIP_SYMBOLS:
        assert getattr(lib, n).argtypes is not None
    csrc = os.path.join(ROOT, "large-steps-pytorch_amd", "csrc")
    for name in ("mip.hip", "textaps.h"):
        src = open(os.path.join(csrc, name)).read()
        assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    assert "mip.hip" in open(os.path.join(csrc, "Makefile")).read()
    # sizes and modes are checked before the device is touched: LS_E_INVALID = -1, LS_E_OVERFLOW = -4
    n = ctypes.c_size_t(0)
    assert lib.ls_mip_workspace_bytes(2, 16, 16, ctypes.byref(n)) == 0 and n.value >= 2 * 4 * 4 * 512
    assert lib.ls_mip_workspace_bytes(0, 16, 16, ctypes.byref(n)) == -1
    assert lib.ls_mip_workspace_bytes(1 << 20, 1 << 10, 1 << 10, ctypes.byref(n)) == -4
    null = ctypes.c_void_p(0)

    def forward(Bt, Ht, Wt, C, Lmax, B, H, W, mode, bnd):
        return lib.ls_mip_forward(null, null, Bt, Ht, Wt, C, Lmax, null, null, null, B, H, W, mode, bnd, null, 0, null)

    assert forward(1, 8, 8, 3, 3, 2, 4, 4, 1, 0) == -1 and "null" in _native.last_error()
    for bad in ((1, 8, 8, 3, 4, 2, 4, 4, 1, 0), (1, 6, 5, 3, 1, 2, 4, 4, 1, 0), (1, 12, 12, 3, 3, 2, 4, 4, 1, 0), (3, 8, 8, 3, 3, 2, 4, 4, 1, 0),
                (1, 8, 8, 3, 3, 2, 4, 4, 2, 0), (1, 8, 8, 3, 3, 2, 4, 4, 1, 3), (1, 8, 8, 33, 3, 2, 4, 4, 1, 0), (1, 8, 8, 3, -1, 2, 4, 4, 1, 0)):
        assert forward(*bad) == -1 and "null" not in _native.last_error(), bad
    assert lib.ls_mip_build(null, 1, 6, 5, 1, 1, null, 0, null) == -1 and "1 or even" in _native.last_error()
    assert lib.ls_mip_fold(null, 1, 8, 8, 1, 2, null, 0, null) == -1
    assert lib.ls_mip_pixel_differentials(null, null, 1, 3, null, 1, 0, 4, null, 0, null) == -1
    assert lib.ls_mip_interpolate_da(null, 2, 3, 1, null, null, 3, 4, 4, null, 1, null, 0, null) == -1
    assert lib.ls_mip_order(null, null, null, 2, 4, 4, 1, 8, 8, 3, 1, 0, null, null, null, 0, 0, null) == -1
    assert lib.ls_mip_backward(null, null, 1, 8, 8, 0, 3, null, null, null, 2, 4, 4, 1, 0, null, null, null, null, null, null, null, null, 0, null) == -1


def test_the_scale_cases_stay_under_the_flag_cap_and_meet_their_conditions():
    """the cases of tests/test_mip_scale_gpu.py, from the statement alone"""
    import texture_cases as tc

    def offsets(shape, Lmax):
        sizes = [shape[0] * max(shape[1] >> l, 1) * max(shape[2] >> l, 1) for l in range(Lmax + 1)]
        return np.cumsum(sizes).tolist()

    for name, (tex_shape, uv_shape, max_level) in tc.MIP_CASES.items():
        tex, uv, da, bias, ml, g = tc.mip_case(name)
        assert tex.shape == tex_shape and uv.shape == uv_shape + (2,) and ml == max_level and g.shape == uv_shape + tex_shape[3:]
        for mode in ms.MODES:
            # one boundary mode is enough: lod, the level choice, `flag` and `two` come from uv_da and the bias alone; the per-level counts
            # checked below are those of clamp (the device test asserts the flag cap again for every boundary mode it runs)
            r = ms.texture(tex, uv, da, bias, g, mode, "clamp", max_level)
            linear = mode == "linear-mipmap-linear"
            assert r.flag.mean() <= 0.02, (name, mode, r.flag.mean())
            assert r.finite.all() and len(r.level_n) == r.Lmax + 1
            # per-level counts: every item is counted once per tap, on its own level
            assert sum(int(n.sum()) for n in r.level_n) == 4 * (int(r.finite.sum()) + int(r.two.sum()))
            if name == "mip_threshold":
                assert not r.flag.any() and da is None and r.Lmax == 5
                n0, n1, n2 = (r.level_n[l][0] for l in range(3))
                assert (n0 == 64).any() and (n0 == 65).any() and n2.max() > 64 and linear == bool(n1.max() > 64)
                assert not any(n.any() for n in r.level_n[3:])
                assert sorted(set(n0.ravel()[:64]) - {0}) == [1, 32, 33, 64, 65, 350]   # level 0's first wave: short, 64, and two long texels
                want = tc.threshold_counts([((m + 1) // 2, i, j) for m, i, j in tc.MIP_THRESHOLD_CLUSTERS], *tex_shape[1:3])
                assert np.array_equal(n0, want) and n0[4, 21] == 20 + 13 and n0[8, 27] == 20 + 12
                assert r.two.sum() == (sum(m // 2 for m, _, _ in tc.MIP_THRESHOLD_CLUSTERS) if linear else 0)
                assert offsets(tex_shape, 5) == [512, 640, 672, 680, 682, 683]          # level 2 lies in the third, partial workgroup
            else:
                assert (r.lod < 0).any() and (r.lod > r.Lmax).any() and (not linear or r.two.mean() > 0.5)
                assert max(int(n.max()) for n in r.level_n) > 64
        nk = tc.mip_keys(tex_shape, r.Lmax)
        if name.startswith("three_pass"):
            assert tc.texture_keys(tex_shape) >= 65536 and nk < 2 ** 24 and tc.radix_passes(nk) == 3
        else:
            assert tc.radix_passes(nk) == 2
        if name.startswith("levels_straddle"):
            # level 1 starts inside a workgroup (on a wave boundary: 2880 = 45 x 64), levels 2 and 3 inside a wave
            assert r.Lmax == 3 and offsets(tex_shape, 3) == [2880, 3600, 3780, 3825] and 2880 % 256 and 3600 % 64 and 3780 % 64
        if name.startswith("deep"):
            assert r.Lmax == 9
            thin = [lv.shape[1] == 1 or lv.shape[2] == 1 for lv in r.levels]
            assert sum(thin) >= 4 and min(lv.shape[1] * lv.shape[2] for lv, t in zip(r.levels, thin) if t) == 1
            assert all(n.any() for n in r.level_n)                                      # every thin level receives gradient of its own


def test_the_bounds_hold_between_two_summation_orders_of_the_statement():
    """as in tests/test_texture_cpu.py: the statement with its pixels reversed differs from itself by far less than the device bound, and
    the bound stays a small fraction of an entry's terms at 861 items on one level-2 texel"""
    import texture_cases as tc
    tex, uv, da, bias, ml, g = tc.mip_case("mip_threshold")
    a = ms.texture(tex, uv, da, bias, g, "linear-mipmap-linear", "clamp", ml)
    b = ms.texture(tex, uv[:, ::-1, ::-1], da, bias[:, ::-1, ::-1], g[:, ::-1, ::-1], "linear-mipmap-linear", "clamp", ml)
    assert np.array_equal(a.grad_tex_n, b.grad_tex_n) and a.level_n[2].max() == 861
    bound = (a.grad_tex_n[..., None] + 16) * ms.U * a.grad_tex_abs + a.grad_tex_lod
    diff = np.abs(a.grad_tex - b.grad_tex)
    assert diff.max() > 0 and np.all(diff <= 1e-6 * bound)
    assert bound.max() > 0 and np.all(bound <= 3e-4 * a.grad_tex_abs)
