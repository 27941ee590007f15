"""
largesteps.render.texture without a device: the numpy statement (tests/texture_statement.py) against central finite differences, against
the plain-torch lookup CPU tensors get and the coordinates the reference hands to dr.texture (tests/golden/reference_render.npz), a
few cases worked by hand, and the public surface (symbols, argument checks, the modes that stay unsupported). And the statement's
scatter against np.add.at (bit for bit), the conditions the cases of tests/texture_cases.py were built for, and the device bound against
two summation orders of the statement itself.
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

import texture_statement as ts  # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32


def _uv_inside_cells(rng, shape, Ht, Wt, linear, lo=-1.5, hi=2.5):
    """fp64 uv in [lo, hi) whose texel-space coordinate keeps 0.1 away from every cell border (x integer: the kink of the bilinear
    lookup, the jump of the nearest one)"""
    out = np.empty(shape + (2,))
    for a, n in ((0, Wt), (1, Ht)):
        cell = rng.integers(int(np.floor(lo * n)), int(np.ceil(hi * n)), shape)
        x = cell + rng.uniform(0.1, 0.9, shape)
        out[..., a] = (x + 0.5) / n if linear else x / n
    return out


@pytest.mark.parametrize("boundary", ts.BOUNDARIES)
@pytest.mark.parametrize("filt", ts.FILTERS)
def test_statement_gradients_match_central_differences(filt, boundary):
    rng = np.random.default_rng(11)
    B, H, W, Ht, Wt, C = 2, 5, 7, 4, 6, 3
    for Bt in (1, B):
        tex = rng.standard_normal((Bt, Ht, Wt, C))
        uv = _uv_inside_cells(rng, (B, H, W), Ht, Wt, filt == "linear")
        g = rng.standard_normal((B, H, W, C))

        def loss(t, c):
            return float((ts.texture(t, c, None, filt, boundary, coords=np.float64).out * g).sum())

        r = ts.texture(tex, uv, g, filt, boundary, coords=np.float64)
        eps = 1e-6
        for trial in range(3):
            dt, dc = rng.standard_normal(tex.shape), rng.standard_normal(uv.shape)
            fd_t = (loss(tex + eps * dt, uv) - loss(tex - eps * dt, uv)) / (2 * eps)
            fd_c = (loss(tex, uv + eps * dc) - loss(tex, uv - eps * dc)) / (2 * eps)
            an_t, an_c = float((r.grad_tex * dt).sum()), float((r.grad_uv * dc).sum())
            assert abs(fd_t - an_t) <= 1e-7 * (np.abs(r.grad_tex_abs * np.abs(dt)).sum() + 1.0), (Bt, trial, fd_t, an_t)
            assert abs(fd_c - an_c) <= 1e-7 * (np.abs(r.grad_uv_abs * np.abs(dc)).sum() + 1.0), (Bt, trial, fd_c, an_c)
            if filt == "nearest":
                assert an_c == 0.0 and fd_c == 0.0
            else:
                assert abs(an_c) > 1e-3
            assert abs(an_t) > 1e-3


def test_statement_linear_wrap_equals_the_plain_torch_lookup():
    """the CPU path of `texture` (the parent's whole implementation) in fp32 against the statement with the same fp32 fractions:
    at most nine fp32 roundings follow them"""
    from largesteps.render import texture
    rng = np.random.default_rng(3)
    golden = np.load(os.path.join(HERE, "golden", "reference_render.npz"))
    cases = [(rng.standard_normal((Bt, Ht, Wt, C)).astype(np.float32), rng.uniform(-2.0, 3.0, (B, 9, 11, 2)).astype(np.float32))
             for Bt, B, Ht, Wt, C in ((1, 3, 5, 8, 3), (2, 2, 7, 3, 4), (1, 1, 1, 1, 1))]
    cases.append((golden["sh_envmap"][None], golden["bg_uvs"]))
    for tex, uv in cases:
        got = texture(torch.from_numpy(tex), torch.from_numpy(uv)).numpy()
        ref = ts.texture(tex, uv).out
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.abs(got - ref).max() <= 16 * U * np.abs(tex).max()


def test_hand_cases():
    tex = np.arange(1.0, 13.0).reshape(1, 3, 4, 1)          # row j holds 4 j + 1 .. 4 j + 4
    # nearest picks the texel under the point
    uv = np.array([[[[0.26, 0.34], [0.99, 0.99], [0.0, 0.0]]]])
    assert ts.texture(tex, uv, None, "nearest", "wrap").out.ravel().tolist() == [6.0, 12.0, 1.0]
    # clamp returns the edge texel left of u = 0 and right of u = 1 (v at the centre of row 1)
    uv = np.array([[[[-0.3, 0.5], [1.7, 0.5], [-5.0, 0.5]]]])
    for filt in ts.FILTERS:
        assert ts.texture(tex, uv, None, filt, "clamp").out.ravel().tolist() == [5.0, 8.0, 5.0]
    # zero: the corner (0, 0) of the texture is a quarter of the corner texel; a point further out reads 0
    uv = np.array([[[[0.0, 0.0], [1.0, 1.0], [-0.2, 0.5]]]])
    assert ts.texture(tex, uv, None, "linear", "zero").out.ravel().tolist() == [0.25, 3.0, 0.0]
    # wrap: the same corner blends the four corner texels
    assert ts.texture(tex, uv[:, :, :1], None, "linear", "wrap").out.item() == (1.0 + 4.0 + 9.0 + 12.0) / 4
    # a texture shared by every image receives the sum of the per-image gradients
    rng = np.random.default_rng(5)
    tex = rng.standard_normal((1, 4, 5, 2))
    uv, g = rng.uniform(-1, 2, (3, 6, 6, 2)), rng.standard_normal((3, 6, 6, 2))
    for filt in ts.FILTERS:
        for boundary in ts.BOUNDARIES:
            shared = ts.texture(tex, uv, g, filt, boundary).grad_tex
            per_image = sum(ts.texture(tex, uv[b:b + 1], g[b:b + 1], filt, boundary).grad_tex for b in range(3))
            np.testing.assert_allclose(shared, per_image, rtol=0, atol=1e-12)
            own = ts.texture(np.repeat(tex, 3, 0), uv, g, filt, boundary).grad_tex
            np.testing.assert_allclose(shared[0], own.sum(0), rtol=0, atol=1e-12)
    # a non-finite coordinate: output 0, no gradient
    uv = np.array([[[[np.nan, 0.5], [0.5, np.inf], [0.5, 0.5]]]])
    r = ts.texture(tex, uv, np.ones((1, 1, 3, 2)), "linear", "wrap")
    assert np.all(r.out[0, 0, :2] == 0) and np.all(r.grad_uv[0, 0, :2] == 0) and r.grad_tex_n.sum() == 4


def test_native_entry_points_are_exported_and_bound():
    from largesteps import _native
    names = ["ls_texture_workspace_bytes", "ls_texture_forward", "ls_texture_order", "ls_texture_backward"]
    assert sorted(n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_texture_")) == sorted(names)
    lib = _native.lib()
    for n in names:
        assert getattr(lib, n).argtypes is not None
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "texture.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    # sizes and modes are checked before the device is touched (no device here): LS_E_INVALID = -1, LS_E_OVERFLOW = -4
    n = ctypes.c_size_t(0)
    assert lib.ls_texture_workspace_bytes(2, 16, 16, ctypes.byref(n)) == 0 and n.value >= 4 * 4 * 512
    assert lib.ls_texture_workspace_bytes(0, 16, 16, ctypes.byref(n)) == -1
    assert lib.ls_texture_workspace_bytes(1 << 20, 1 << 10, 1 << 10, ctypes.byref(n)) == -4
    null = ctypes.c_void_p(0)

    def forward(Bt, Ht, Wt, C, B, H, W, filt, bnd):
        return lib.ls_texture_forward(null, Bt, Ht, Wt, C, null, B, H, W, filt, bnd, null, 0, null)

    assert forward(1, 4, 4, 3, 2, 8, 8, 1, 0) == -1 and "null" in _native.last_error()
    for bad in ((3, 4, 4, 3, 2, 8, 8, 1, 0), (1, 0, 4, 3, 2, 8, 8, 1, 0), (1, 4, 8193, 3, 2, 8, 8, 1, 0), (1, 4, 4, 33, 2, 8, 8, 1, 0),
                (1, 4, 4, 3, 2, 8, 8, 2, 0), (1, 4, 4, 3, 2, 8, 8, 1, 3), (1, 4, 4, 3, 2, 0, 8, 1, 0)):
        assert forward(*bad) == -1 and "null" not in _native.last_error(), bad
    assert lib.ls_texture_order(null, 2, 8, 8, 1, 4, 4, 1, 5, null, null, null, 0, 0, null) == -1
    assert lib.ls_texture_backward(null, 1, 4, 4, 0, null, 2, 8, 8, 1, 0, null, null, null, null, null, 0, null) == -1


def test_argument_errors_come_before_any_device_call():
    from largesteps.render import texture
    tex, uv = torch.zeros(1, 4, 4, 3), torch.zeros(2, 5, 5, 2)
    with pytest.raises(TypeError):
        texture(tex.double(), uv)
    with pytest.raises(TypeError):
        texture(tex, uv.half())
    with pytest.raises(TypeError):
        texture(tex.numpy(), uv)
    with pytest.raises(ValueError):
        texture(tex[0], uv)
    with pytest.raises(ValueError):
        texture(tex, torch.zeros(2, 5, 5, 3))
    with pytest.raises(ValueError, match="batches"):
        texture(torch.zeros(3, 4, 4, 3), uv)
    with pytest.raises(ValueError, match="8192"):
        texture(torch.zeros(1, 1, 8193, 1), uv)
    with pytest.raises(ValueError, match="channels"):
        texture(torch.zeros(1, 2, 2, 33), uv)
    with pytest.raises(ValueError):
        texture(tex, torch.zeros(0, 5, 5, 2))
    with pytest.raises(ValueError, match="filter_mode"):
        texture(tex, uv, filter_mode="cubic")
    with pytest.raises(ValueError, match="boundary_mode"):
        texture(tex, uv, boundary_mode="mirror")
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="is on"):
            texture(tex.cuda(), uv)


def test_unsupported_modes_still_raise_and_cpu_tensors_keep_the_plain_lookup():
    from largesteps.render import texture
    tex, uv = torch.rand(1, 4, 4, 3), torch.rand(2, 5, 5, 2)
    for mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        with pytest.raises(NotImplementedError):
            texture(tex, uv, filter_mode=mode)
    with pytest.raises(NotImplementedError):
        texture(tex, uv, boundary_mode="cube")
    # accepted and ignored, as before
    a = texture(tex, uv, uv_da=torch.zeros(2, 5, 5, 4), mip_level_bias=torch.zeros(2, 5, 5), mip=None, filter_mode="auto", max_mip_level=3)
    assert torch.equal(a, texture(tex, uv)) and not a.requires_grad
    # every other mode needs the device
    for kw in (dict(filter_mode="nearest"), dict(boundary_mode="clamp"), dict(boundary_mode="zero")):
        with pytest.raises(NotImplementedError, match="HIP device"):
            texture(tex, uv, **kw)


# ---- the statement's scatter, and the cases of tests/test_texture_scale_gpu.py ------------------------------------------------------------
def _add_at_scatter(at, term, shape):
    """texture_statement._scatter as it was first written: np.add.at into zeros, term by term"""
    size, C = shape[0] * shape[1] * shape[2], shape[3]
    grad, grad_abs, n = np.zeros((size, C)), np.zeros((size, C)), np.zeros(size, dtype=np.int64)
    np.add.at(grad, at, term)
    np.add.at(grad_abs, at, np.abs(term))
    np.add.at(n, at, 1)
    return grad.reshape(shape), grad_abs.reshape(shape), n.reshape(shape[:3])


def _small_cases():
    """the inputs of the tests above: (tex, uv, g)"""
    rng = np.random.default_rng(11)
    B, H, W, Ht, Wt, C = 2, 5, 7, 4, 6, 3
    for linear in (False, True):
        for Bt in (1, B):
            yield rng.standard_normal((Bt, Ht, Wt, C)), _uv_inside_cells(rng, (B, H, W), Ht, Wt, linear), rng.standard_normal((B, H, W, C))
    rng = np.random.default_rng(3)
    golden = np.load(os.path.join(HERE, "golden", "reference_render.npz"))
    cases = [(rng.standard_normal((Bt, Ht, Wt, C)).astype(np.float32), rng.uniform(-2.0, 3.0, (B, 9, 11, 2)).astype(np.float32))
             for Bt, B, Ht, Wt, C in ((1, 3, 5, 8, 3), (2, 2, 7, 3, 4), (1, 1, 1, 1, 1))]
    cases.append((golden["sh_envmap"][None], golden["bg_uvs"]))
    for tex, uv in cases:
        yield tex, uv, rng.standard_normal(uv.shape[:3] + (tex.shape[3],))
    rng = np.random.default_rng(5)
    yield rng.standard_normal((1, 4, 5, 2)), rng.uniform(-1, 2, (3, 6, 6, 2)), rng.standard_normal((3, 6, 6, 2))
    yield rng.standard_normal((1, 4, 5, 2)), np.array([[[[np.nan, 0.5], [0.5, np.inf], [0.5, 0.5]]]]), np.ones((1, 1, 3, 2))


def test_the_bincount_scatter_is_the_add_at_scatter_bit_for_bit(monkeypatch):
    fast = [[ts.texture(tex, uv, g, f, b, coords=c) for f in ts.FILTERS for b in ts.BOUNDARIES for c in (np.float32, np.float64)]
            for tex, uv, g in _small_cases()]
    monkeypatch.setattr(ts, "_scatter", _add_at_scatter)
    slow = [[ts.texture(tex, uv, g, f, b, coords=c) for f in ts.FILTERS for b in ts.BOUNDARIES for c in (np.float32, np.float64)]
            for tex, uv, g in _small_cases()]
    assert len(fast) == 10
    for rf, rs_ in zip(fast, slow):
        for x, y in zip(rf, rs_):
            assert x.grad_tex_n.dtype == y.grad_tex_n.dtype and x.grad_tex.shape == y.grad_tex.shape
            assert np.array_equal(x.grad_tex_n, y.grad_tex_n) and x.grad_tex_n.sum() > 0
            assert np.array_equal(x.grad_tex, y.grad_tex) and np.array_equal(x.grad_tex_abs, y.grad_tex_abs)


def test_the_scale_cases_meet_their_conditions():
    import texture_cases as tc
    assert [tc.radix_passes(nk) for nk in (0, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 3)] == [1, 1, 2, 2, 3, 3, 4, 4]
    for name, (tex_shape, uv_shape, modes) in tc.TEXTURE_CASES.items():
        nk = tc.texture_keys(tex_shape)
        assert set(modes) <= set(tc.ALL_MODES)
        tex, uv, g = tc.texture_case(name)
        assert tex.shape == tex_shape and uv.shape == uv_shape + (2,) and g.shape == uv_shape + tex_shape[3:]
        assert tex.dtype == uv.dtype == g.dtype == np.float32
        if name != "threshold":                     # every boundary rule fires on both axes
            assert uv.min() < -1.4 and uv.max() > 2.4
        if name != "four_pass_4096_c1":
            assert modes == tc.ALL_MODES
        else:                                       # 16.7 M texels: one statement call, the mode whose border texels pile up
            r = ts.texture(tex, uv, g, "linear", "clamp")
            assert r.grad_tex.shape == tex_shape and r.grad_tex_n.dtype == np.int64 and r.finite.all()
            assert r.grad_tex_n.sum() == 4 * uv[..., 0].size and r.grad_tex_n.max() > 700
            assert r.grad_tex_n[0, 1:-1, 1:-1].max() <= 4 and (r.grad_tex_n[0, 1:-1, 1:-1] > 0).sum() > 200   # inside: a few texels, a few items each
        if name.startswith("three_pass"):
            assert 65536 <= nk < 2 ** 24 and tc.radix_passes(nk) == 3
        if name.startswith("four_pass"):
            assert nk == 4097 ** 2 >= 2 ** 24 and tc.radix_passes(nk) == 4 and modes == (("linear", "wrap"), ("linear", "clamp"))
    assert tc.TEXTURE_CASES["wide_300x5_c3"][0][2] + 1 > 255 and 5 * 300 == 5 * 256 + 220
    assert tc.TEXTURE_CASES["three_pass_own_b4_128x128_c4"][0] == (4, 128, 128, 4) and tc.TEXTURE_CASES["three_pass_own_b4_128x128_c4"][1][0] == 4
    assert tc.TEXTURE_CASES["c32"][0][3] == 32 and tc.TEXTURE_CASES["c5"][0][3] == 5

    # threshold: the counts the layout promises, where it promises them
    Bt, Ht, Wt, C = tc.THRESHOLD_SHAPE
    assert Ht * Wt == 960 and Ht * Wt - 3 * 256 == 192
    cl = tc.THRESHOLD_CLUSTERS
    single = [c for c in cl if c[0] not in (40, 25, 24)]
    assert sorted(m for m, _, _ in single) == [1, 63, 64, 65, 65, 66, 127, 128, 129, 700]
    for a, (_, i, j) in enumerate(cl):              # cells at least two texels apart, but for the two pairs; none touches the border
        assert 1 <= i < Wt - 2 and 0 <= j < Ht - 2
        for m2, i2, j2 in cl[a + 1:]:
            assert abs(i - i2) >= 2 or abs(j - j2) >= 2 or (j == j2 and abs(i - i2) == 1 and m2 in (25, 24))
    want = tc.threshold_counts(cl, Ht, Wt)
    for boundary in ts.BOUNDARIES:
        tex, uv, g = tc.texture_case("threshold", "linear")
        r = ts.texture(tex, uv, g, "linear", boundary)
        assert np.array_equal(r.grad_tex_n[0], want)
        flat = r.grad_tex_n[0].ravel()
        for m in (1, 63, 64, 65, 66, 127, 128, 129, 700):
            assert (flat == m).any(), m
        assert sorted(set(flat[:64]) - {0}) == [1, 64, 65, 129]                  # one wave: short, exactly 64, and two long texels
        assert (flat[768:] == 65).sum() == 4 and (flat[896:] == 65).sum() == 2  # long texels in the last, partial workgroup and in its last wave
        assert r.grad_tex_n[0, 10, 21] == 40 + 25 and r.grad_tex_n[0, 14, 31] == 40 + 24 and r.grad_tex_n[0, 10, 20] == 40
        # strictly inside the cells: 0.1 of a texel from every border, in the fp32 arithmetic of the device
        x, y = uv[..., 0] * np.float32(Wt) - np.float32(0.5), uv[..., 1] * np.float32(Ht) - np.float32(0.5)
        for f in (x - np.floor(x), y - np.floor(y)):
            assert f.min() > 0.09 and f.max() < 0.91
        tex, uv, g = tc.texture_case("threshold", "nearest")
        n = ts.texture(tex, uv, g, "nearest", boundary).grad_tex_n[0]
        assert sorted(n[n > 0]) == sorted(m for m, _, _ in cl) and all(n[j, i] == m for m, i, j in cl)
        assert np.array_equal(uv[..., 0] * np.float32(Wt), np.floor(uv[..., 0] * np.float32(Wt)) + np.float32(0.5))


@pytest.mark.parametrize("name,filt,boundary", [("threshold", "linear", "wrap"), ("threshold", "nearest", "zero"), ("constant_uv", "linear", "wrap"),
                                                ("three_pass_255x257_c3", "linear", "clamp")])
def test_the_bounds_hold_between_two_summation_orders_of_the_statement(name, filt, boundary):
    """the statement with fp32 coordinates, its pixels taken in reverse, is the same sum in another order: the two differ (fp64 is
    not associative) by far less than the device bound, which at 700, 2048 and 4690 terms is still a small fraction of the entry's
    terms -- the bound neither fails a correct sum nor admits a wrong term"""
    import texture_cases as tc
    if name == "constant_uv":
        rng = np.random.default_rng(0)
        tex, g = rng.standard_normal((1, 6, 4, 3)).astype(np.float32), rng.standard_normal((2, 32, 32, 3)).astype(np.float32)
        uv = np.broadcast_to(np.float32([0.62, 0.4]), (2, 32, 32, 2)).copy()
    else:
        tex, uv, g = tc.texture_case(name, filt)
    a = ts.texture(tex, uv, g, filt, boundary, coords=np.float32)
    b = ts.texture(tex, uv[:, ::-1, ::-1], g[:, ::-1, ::-1], filt, boundary, coords=np.float32)
    assert np.array_equal(a.grad_tex_n, b.grad_tex_n) and a.grad_tex_n.max() >= 700
    bound = (a.grad_tex_n[..., None] + 16) * U * a.grad_tex_abs
    diff = np.abs(a.grad_tex - b.grad_tex)
    assert (diff.max() > 0 or filt == "nearest") and np.all(diff <= 1e-6 * bound)       # (nearest: sums of fp32 numbers, exact in fp64)
    hit = a.grad_tex_n > 0
    assert np.all(bound[hit] > 0) and not bound[~hit].any()
    assert np.all(bound <= 3e-4 * a.grad_tex_abs)               # (4690 + 16) 2^-24 = 2.8e-4: dropping one term of a long texel is caught
    assert np.array_equal(a.out, b.out[:, ::-1, ::-1]) and np.array_equal(a.grad_uv, b.grad_uv[:, ::-1, ::-1])
