"""
largesteps.render.texture(..., boundary_mode='cube') without a device: the numpy statement (tests/cube_statement.py) against central
differences of itself, its properties (continuity across the 12 edges and at the 8 corners, a gradient perpendicular to the direction,
weights that sum to one, the tie rule, directions without a face), and the public surface (symbols, the size and mode checks of the
native entry points through NULL-pointer calls, argument errors that need no device).
"""
import ctypes
import itertools
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

import cube_statement as cs  # noqa: E402
from cube_cases import directions_inside_cells as _directions_inside_cells  # noqa: E402

CUBE_SYMBOLS = ["ls_cube_workspace_bytes", "ls_cube_forward", "ls_cube_order", "ls_cube_backward"]
EDGES = [(a, b, sa, sb) for a, b in ((0, 1), (0, 2), (1, 2)) for sa in (1.0, -1.0) for sb in (1.0, -1.0)]
CORNERS = list(itertools.product((1.0, -1.0), repeat=3))


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("filt", cs.FILTERS)
def test_statement_gradients_match_central_differences(filt, n):
    rng = np.random.default_rng(100 + n)
    C, eps = 3, 1e-6
    uv = _directions_inside_cells(rng, n, filt == "linear")
    P = uv.shape[2]
    tex = rng.standard_normal((1, 6, n, n, C))
    g = rng.standard_normal((1, 1, P, C))
    r = cs.cube(tex, uv, g, filt, coords=np.float64)
    assert r.finite.all() and set(r.face.ravel()) == set(range(6))
    if filt == "linear":            # the inputs do reach the seams and the corners
        assert (r.drop >= 0).sum() >= 6 * 8
        if n >= 2:
            assert (~r.inside & (r.drop < 0)).sum() >= 6 * 16 and r.inside.sum() >= 40
        else:                       # one texel a face: every pixel has one tap inside, two across an edge and one beyond a corner
            assert (r.drop >= 0).all()
    for trial in range(3):
        dt, dc = rng.standard_normal(tex.shape), rng.standard_normal(uv.shape)
        # tex: the lookup is linear in it
        fd_t = float(((cs.cube(tex + eps * dt, uv, None, filt, np.float64).out - cs.cube(tex - eps * dt, uv, None, filt, np.float64).out) * g).sum()) / (2 * eps)
        an_t = float((r.grad_tex * dt).sum())
        assert abs(fd_t - an_t) <= 1e-7 * ((r.grad_tex_abs * np.abs(dt)).sum() + 1.0), (trial, fd_t, an_t)
        assert abs(an_t) > 1e-3
        # uv: leave out only pixels whose stencil straddles a face boundary or an integer of x or y
        rp, rm = cs.cube(tex, uv + eps * dc, None, filt, np.float64), cs.cube(tex, uv - eps * dc, None, filt, np.float64)
        keep = np.ones(r.face.shape, bool)
        for q in (rp, rm):
            keep &= (q.face == r.face) & (q.i0 == r.i0) & (q.j0 == r.j0)
        left_out = 1.0 - keep.mean()
        assert left_out < 0.05, left_out
        fd_c = float((((rp.out - rm.out) * g).sum(-1) * keep).sum()) / (2 * eps)
        an_c = float(((r.grad_uv * dc).sum(-1) * keep).sum())
        assert abs(fd_c - an_c) <= 1e-6 * ((r.grad_uv_abs * np.abs(dc)).sum() + 1.0), (trial, fd_c, an_c)
        if filt == "nearest":
            assert an_c == 0.0 and fd_c == 0.0
        else:
            assert abs(an_c) > 1e-3


def _edge_points(rng, m):
    """m points on each of the 12 edges: (12 m, 3) fp64 with the axis across which the edge is crossed"""
    pts, axes = [], []
    for a, b, sa, sb in EDGES:
        d = np.empty((m, 3))
        d[:, a], d[:, b], d[:, 3 - a - b] = sa, sb, rng.uniform(-1, 1, m)
        pts.append(d); axes.append(np.full(m, b))
    return np.concatenate(pts), np.concatenate(axes)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_the_linear_lookup_is_continuous_across_every_edge_and_at_every_corner(n):
    """d +- eps across an edge lies on two faces: the lookups differ by O(eps n max|tex|). A wrong neighbour, a flipped orientation or a
    wrong border row would differ by O(max|tex|)."""
    rng = np.random.default_rng(n)
    tex = rng.standard_normal((1, 6, n, n, 2))
    eps = 1e-7
    pts, axes = _edge_points(rng, 64)
    corners = np.repeat(np.array(CORNERS), 3, axis=0)
    pts, axes = np.concatenate([pts, corners]), np.concatenate([axes, np.tile(np.arange(3), 8)])
    step = np.zeros_like(pts)
    step[np.arange(len(pts)), axes] = eps
    lo = cs.cube(tex, (pts * (1 - step))[None, None], None, "linear", np.float64)
    hi = cs.cube(tex, (pts * (1 + step))[None, None], None, "linear", np.float64)
    on = cs.cube(tex, pts[None, None], None, "linear", np.float64)
    assert (lo.face != hi.face).sum() >= 12 * 64                                # the pairs do straddle an edge
    bound = 20 * eps * n * np.abs(tex).max()
    assert np.abs(lo.out - hi.out).max() <= bound and np.abs(lo.out - on.out).max() <= bound
    assert np.abs(on.out).max() > 0.1
    assert (on.drop[0, 0, -24:] >= 0).all()                                      # a corner drops a tap


def test_statement_properties():
    rng = np.random.default_rng(4)
    for n in (1, 2, 5):
        uv = np.concatenate([_directions_inside_cells(rng, n, True), rng.standard_normal((1, 1, 300, 3))], axis=2)
        P = uv.shape[2]
        tex, g = rng.standard_normal((1, 6, n, n, 3)), rng.standard_normal((1, 1, P, 3))
        r = cs.cube(tex, uv, g, "linear", np.float64)
        # the gradient is perpendicular to the direction
        dot = (r.grad_uv * uv).sum(-1)
        assert np.all(np.abs(dot) <= 1e-12 * (r.grad_uv_abs * np.abs(uv)).sum(-1) + 1e-300) and np.abs(r.grad_uv).max() > 1e-2
        # a constant texture gives that constant everywhere, corners included: the weights sum to 1, and every term lands on a texel
        for filt in cs.FILTERS:
            c = cs.cube(np.full((1, 6, n, n, 1), 3.25), uv, np.ones((1, 1, P, 1)), filt, np.float64)
            assert np.abs(c.out - 3.25).max() <= 1e-14 and np.abs(c.out_abs - 3.25).max() <= 1e-14
            assert abs(c.grad_tex.sum() - P) <= 1e-10 and np.abs(c.grad_uv).max() <= 1e-12 * n
        # the length of the direction does not matter
        r2 = cs.cube(tex, 7.5 * uv, None, "linear", np.float64)
        assert np.abs(r2.out - r.out).max() <= 1e-12
        # a texture per image and a shared one
        own = cs.cube(np.repeat(tex, 2, 0), np.concatenate([uv, uv[:, :, ::-1]]), np.concatenate([g, g]), "linear", np.float64)
        shared = cs.cube(tex, np.concatenate([uv, uv[:, :, ::-1]]), np.concatenate([g, g]), "linear", np.float64)
        np.testing.assert_allclose(own.grad_tex.sum(0), shared.grad_tex[0], rtol=0, atol=1e-11)


def test_the_tie_rule_and_directions_without_a_face():
    tex = np.arange(6.0 * 4).reshape(1, 6, 2, 2, 1)
    d = np.array([[1, 1, 0.3], [-1, 1, 0], [0.2, 1, 1], [0.2, -1, 1], [1, 1, 1], [-1, -1, -1], [0.5, -1, -1], [0, 0.5, 0.5], [0, 0, -2],
                  [-1, -1, 1], [0.3, -0.3, 0.1]])
    for coords in (np.float32, np.float64):
        r = cs.cube(tex, d[None, None], None, "nearest", coords)
        assert r.face.ravel().tolist() == [0, 1, 2, 3, 0, 1, 3, 2, 5, 1, 0]
    # hand cases, nearest: +x looks along -z for s and -y for t
    r = cs.cube(tex, np.array([[[[1.0, 0.5, 0.5], [1.0, -0.5, -0.5], [0.1, 0.2, -3.0]]]]), None, "nearest")
    assert r.out.ravel().tolist() == [0.0, 3.0, 20.0 + 2.0 * 0 + 0]             # (+x: s < .5, t < .5) (+x: s > .5, t > .5) (-z: sc = -x < 0, tc = -y < 0)
    # the centre of a face reads the mean of its four texels at n = 2
    r = cs.cube(tex, np.array([[[[0.0, 3.0, 0.0]]]]), None, "linear")
    assert r.out.item() == (8 + 9 + 10 + 11) / 4 and r.inside.all()
    # no face: non-finite components and the zero vector
    bad = np.array([[[[np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [-0.0, 0.0, -0.0], [1, 2, 3]]]])
    for filt in cs.FILTERS:
        for coords in (np.float32, np.float64):
            r = cs.cube(tex, bad, np.ones((1, 1, 6, 1)), filt, coords)
            assert r.finite.ravel().tolist() == [False] * 5 + [True]
            assert np.all(r.out[0, 0, :5] == 0) and np.all(r.grad_uv[0, 0, :5] == 0) and r.out[0, 0, 5] != 0
            assert r.grad_tex_n.sum() == (4 if filt == "linear" else 1)


def test_native_entry_points_are_exported_and_bound():
    from largesteps import _native
    assert sorted(n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_cube_")) == sorted(CUBE_SYMBOLS)
    lib = _native.lib()
    for n in CUBE_SYMBOLS:
        assert getattr(lib, n).argtypes is not None
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "cube.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    assert lib.ls_version() == 110
    # sizes and modes are checked before the device is touched (no device here): LS_E_INVALID = -1, LS_E_OVERFLOW = -4
    nb = ctypes.c_size_t(0)
    assert lib.ls_cube_workspace_bytes(2, 16, 16, ctypes.byref(nb)) == 0 and nb.value >= 4 * 4 * 4 * 512
    assert lib.ls_cube_workspace_bytes(0, 16, 16, ctypes.byref(nb)) == -1
    assert lib.ls_cube_workspace_bytes(2, 16, 16, None) == -1
    assert lib.ls_cube_workspace_bytes(1 << 20, 1 << 10, 1 << 10, ctypes.byref(nb)) == -4
    assert lib.ls_cube_workspace_bytes(1, 1 << 15, 1 << 14, ctypes.byref(nb)) == -4          # 4 B H W = 2^31
    assert lib.ls_cube_workspace_bytes(1, 1 << 14, 1 << 14, ctypes.byref(nb)) == 0
    null = ctypes.c_void_p(0)

    def forward(Bt, n, C, B, H, W, filt):
        return lib.ls_cube_forward(null, Bt, n, C, null, B, H, W, filt, null, 0, null)

    assert forward(1, 4, 3, 2, 8, 8, 1) == -1 and "null" in _native.last_error()
    assert forward(2, 1, 32, 2, 1, 1, 0) == -1 and "null" in _native.last_error()
    for bad in ((3, 4, 3, 2, 8, 8, 1), (1, 0, 3, 2, 8, 8, 1), (1, 8193, 3, 2, 8, 8, 1), (1, 4, 33, 2, 8, 8, 1), (1, 4, 0, 2, 8, 8, 1),
                (1, 4, 3, 2, 8, 8, 2), (1, 4, 3, 2, 8, 8, -1), (1, 4, 3, 2, 0, 8, 1), (0, 4, 3, 2, 8, 8, 1)):
        assert forward(*bad) == -1 and "null" not in _native.last_error(), bad
    assert forward(8, 8192, 3, 8, 8, 8, 1) == -4                                 # 6 Bt n^2 = 3 * 2^30
    assert forward(1, 4, 3, 1, 1 << 15, 1 << 14, 1) == -4                        # 4 B H W = 2^31
    assert lib.ls_cube_order(null, 2, 8, 8, 1, 4, 5, null, null, null, 0, 0, null) == -1 and "null" not in _native.last_error()
    assert lib.ls_cube_order(null, 2, 8, 8, 1, 4, 1, null, null, null, 0, 0, null) == -1 and "null" in _native.last_error()
    assert lib.ls_cube_backward(null, 1, 4, 0, null, 2, 8, 8, 1, null, null, null, null, null, 0, null) == -1 and "null" not in _native.last_error()
    assert lib.ls_cube_backward(null, 1, 4, 3, null, 2, 8, 8, 1, null, null, null, null, null, 0, null) == -1 and "null" in _native.last_error()
    # the 2-D lookup keeps rejecting boundary 3
    assert lib.ls_texture_forward(null, 1, 4, 4, 3, null, 2, 8, 8, 1, 3, null, 0, null) == -1 and "null" not in _native.last_error()


def test_argument_errors_that_need_no_device():
    import largesteps.render as dr
    cube, dirs = torch.zeros(1, 6, 4, 4, 3), torch.zeros(2, 5, 5, 3)
    # tensors that are not on a HIP device: before any shape check
    for tex, uv in ((torch.zeros(1, 4, 4, 3), torch.zeros(2, 5, 5, 2)), (cube, dirs), (cube.double(), dirs[0])):
        for filt in ("nearest", "linear", "auto"):
            with pytest.raises(NotImplementedError, match="HIP device"):
                dr.texture(tex, uv, filter_mode=filt, boundary_mode="cube")
    for mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        with pytest.raises(NotImplementedError):
            dr.texture(cube, dirs, filter_mode=mode, boundary_mode="cube")
    with pytest.raises(TypeError):
        dr.texture(cube.numpy(), dirs.numpy(), boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="mipmapped cube maps"):
        dr.texture_construct_mip(cube, cube_mode=True)
    # the docs say what is in and what is out
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "mipmapped cube maps" in design and "cube maps of `texture`" not in design
