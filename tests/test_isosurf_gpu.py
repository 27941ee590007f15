"""
largesteps.levelset on the device (csrc/isosurf.hip) against tests/isosurf_statement.py. The statement forms every fp32 and fp64 number
with the operations of the device code in its order and numbers vertices and faces by the same rule, so the device must return exactly
the statement's arrays: V, E, F, and gS for a seeded gV, bit for bit, no tolerance anywhere. Every grid is small; 33^3 has more nodes
and cubes than one chunk of the scan.
"""
import math

import numpy as np
import pytest
import torch

import isosurf_statement as st

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def run(dev, S, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, seed=0):
    """the device's (V, E, F, gS, gV) for the contiguous fp32 array S, as numpy"""
    from largesteps.levelset import isosurface
    t = torch.from_numpy(np.ascontiguousarray(S, dtype=F32)).to(dev).requires_grad_()
    V, F, E = isosurface(t, iso, origin, spacing, return_edges=True)
    assert V.dtype == torch.float32 and F.dtype == torch.int64 and E.dtype == torch.int64
    assert V.requires_grad and not F.requires_grad and not E.requires_grad
    gV = torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(V.shape)).astype(F32)).to(dev)
    gS, = torch.autograd.grad((V * gV).sum(), t)
    return tuple(x.detach().cpu().numpy() for x in (V, E, F, gS, gV))


def check(dev, S, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0):
    S = np.ascontiguousarray(S, dtype=F32)
    V, E, F, gS, gV = run(dev, S, iso, origin, spacing)
    Vs, Es, Fs = st.extract(S, iso, origin, spacing)
    assert V.shape == Vs.shape and F.shape == Fs.shape
    assert np.array_equal(V.view(np.int32), Vs.view(np.int32))
    assert np.array_equal(E, Es) and np.array_equal(F, Fs)
    g = st.grad_S(S, iso, spacing, gV)
    assert gS.shape == S.shape and np.array_equal(gS.view(np.int32), g.view(np.int32))
    return V, E, F


def test_one_cube_all_256_sign_patterns(dev):
    rng = np.random.default_rng(1)
    faces = 0
    for pattern in range(256):
        sign = np.array([-1.0 if pattern >> c & 1 else 1.0 for c in range(8)])
        S = (sign * rng.uniform(0.1, 2.0, 8)).reshape(2, 2, 2)
        faces += check(dev, S, origin=(0.5, -1.0, 2.0), spacing=(0.5, 2.0, 1.25))[2].shape[0]
    assert faces == 256 * 6 * 20 // 16                     # per tet: 2 of 16 cases are empty, 8 give one face and 6 give two


@pytest.mark.parametrize("shape", [(3, 2, 2), (2, 5, 3), (5, 6, 7), (17, 9, 33)])
def test_shapes_off_any_tile(dev, shape):
    S = np.random.default_rng(sum(shape)).standard_normal(shape)
    V, E, F = check(dev, S, iso=0.1)
    assert V.shape[0] > 0 and F.shape[0] > 0


@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 1, 4), (4, 4, 1)])
def test_a_side_of_one_gives_empty_output(dev, shape):
    V, E, F = check(dev, np.random.default_rng(2).standard_normal(shape))
    assert V.shape == (0, 3) and E.shape == (0,) and F.shape == (0, 3)


@pytest.mark.parametrize("value", [-1.0, 1.0])
def test_all_low_and_all_high_give_empty_output(dev, value):
    V, E, F = check(dev, np.full((5, 4, 6), value))
    assert V.shape == (0, 3) and E.shape == (0,) and F.shape == (0, 3)


def test_a_surface_leaving_the_grid(dev):
    V, E, F = check(dev, st.sphere_sdf((8, 7, 9), (1.3, 3.1, 7.6), 3.4))
    assert st.boundary_edges(F).shape[0] > 0


def test_integer_values_with_iso_on_a_value(dev):
    S = np.random.default_rng(3).integers(-2, 3, (6, 7, 5))
    for iso in (1.0, 0.0, -2.0, 3.0):
        check(dev, S, iso=iso)


def test_nan_and_inf_nodes(dev):
    S = np.random.default_rng(4).standard_normal((7, 6, 8)).astype(F32)
    S[2, 3, 4] = np.nan
    S[0, 0, 0] = np.inf
    S[6, 5, 7] = -np.inf
    S[4, 1, 1] = np.nan
    V, E, F = check(dev, S)
    assert np.isfinite(V).all() and F.shape[0] > 0
    check(dev, np.full((3, 3, 3), np.nan))


def test_non_contiguous_field_and_numpy_input(dev):
    from largesteps.levelset import isosurface
    base = np.random.default_rng(5).standard_normal((7, 6, 5)).astype(F32)
    S = np.ascontiguousarray(base.transpose(2, 1, 0))
    Vs, Es, Fs = st.extract(S, 0.2)
    leaf = torch.from_numpy(base).to(dev).requires_grad_()
    view = leaf.permute(2, 1, 0)
    assert not view.is_contiguous()
    V, F, E = isosurface(view, 0.2, return_edges=True)
    gV = torch.from_numpy(np.random.default_rng(6).standard_normal(Vs.shape).astype(F32)).to(dev)
    (V * gV).sum().backward()
    assert np.array_equal(V.detach().cpu().numpy().view(np.int32), Vs.view(np.int32))
    assert np.array_equal(E.cpu().numpy(), Es) and np.array_equal(F.cpu().numpy(), Fs)
    g = st.grad_S(S, 0.2, 1.0, gV.cpu().numpy())
    assert np.array_equal(leaf.grad.cpu().numpy().view(np.int32), np.ascontiguousarray(g.transpose(2, 1, 0)).view(np.int32))
    out = isosurface(S.astype(np.float64), 0.2)
    assert len(out) == 2 and all(isinstance(x, np.ndarray) for x in out)
    assert np.array_equal(out[0].view(np.int32), Vs.view(np.int32)) and np.array_equal(out[1], Fs)
    V2, F2 = isosurface(view.detach(), 0.2)                    # no grad asked: the same arrays
    assert not V2.requires_grad and torch.equal(bits(V2), bits(V.detach())) and torch.equal(F2, F)


def test_origin_and_anisotropic_spacing(dev):
    S = st.sphere_sdf((9, 8, 7), (4.2, 3.6, 3.1), 2.4)
    check(dev, S, origin=(-3.25, 100.5, 0.1), spacing=(0.1, 2.5, 1.0 / 3.0))
    check(dev, S, iso=0.3, origin=(1e-3, -1e3, 7.0), spacing=0.37)


def test_more_than_one_scan_chunk_and_reproducible(dev):
    S = st.sphere_sdf((33, 33, 33), (15.7, 16.2, 16.4), 11.3) + 0.2 * np.random.default_rng(7).standard_normal((33, 33, 33))
    assert S.size > 2048 and 32 ** 3 > 2048
    check(dev, S)
    a, b = run(dev, S), run(dev, S)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32) if x.dtype == F32 else x, y.view(np.int32) if y.dtype == F32 else y)


def test_a_captured_backward_replays_bitwise(dev):
    from largesteps.levelset import isosurface
    Sn = st.sphere_sdf((12, 12, 12), (5.3, 5.8, 5.6), 3.96)
    S = torch.from_numpy(Sn).to(dev).requires_grad_()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        V, F = isosurface(S)                                     # the forward synchronises: eager, on the stream of the capture
        G = torch.from_numpy(np.random.default_rng(8).standard_normal(tuple(V.shape)).astype(F32)).to(dev)

        def backward():
            return torch.autograd.grad((V * G).sum(), S, retain_graph=True)[0]
        eager = backward().clone()                               # the warm-up
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = backward()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(bits(eager), bits(out))
    assert np.array_equal(eager.cpu().numpy().view(np.int32), st.grad_S(Sn, 0.0, 1.0, G.cpu().numpy()).view(np.int32))


def test_the_device_sphere_is_closed_oriented_and_remeshable(dev):
    from largesteps.levelset import isosurface
    from largesteps.remesh import remesh_botsch
    S = st.sphere_sdf((12, 12, 12), (5.3, 5.8, 5.6), 0.33 * 12)
    V, F = isosurface(torch.from_numpy(S).to(dev))
    v, f = V.cpu().numpy(), F.cpu().numpy()
    assert st.boundary_edges(f).shape[0] == 0 and st.euler(v, f) == 2 and st.signed_volume(v, f) > 0
    # its constructor is the project's own check for an edge-manifold, consistently oriented mesh with one fan per vertex
    v2, f2 = remesh_botsch(V, F, 1, 1.0, True)
    assert v2.shape[0] > 0 and f2.shape[0] > 0 and torch.isfinite(v2).all()


def test_repair_of_two_spheres_that_cut_through_each_other(dev):
    """h = 3 / 16 and the default padding meet the condition on the input that tests/test_isosurf_cpu.py checks on the statement's own
    pipeline: no grid node on the mesh, no t of exactly 0 or 1, no reported pair. A point farther than 2 h from the input surface is on
    the same side of both surfaces: every cube within sqrt(3) h of it has all its corners on the point's side and emits nothing, so the
    result does not come between the point and the region it lies in."""
    import selfx_statement as sx
    from largesteps.distance import MeshDistance
    from largesteps.levelset import remesh_level_set
    v, f = sx.two_spheres()
    h = 0.1875
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    with MeshDistance(tv, tf) as before:
        assert int(before.count_self_intersections()) == 94
        V2, F2 = remesh_level_set(tv, tf, h, beta=math.inf)
        v2, f2 = V2.cpu().numpy(), F2.cpu().numpy()
        assert st.boundary_edges(f2).shape[0] == 0 and st.euler(v2, f2) == 2 and st.signed_volume(v2, f2) > 0
        with MeshDistance(V2, F2) as after:
            assert int(after.count_self_intersections()) == 0
            rng = np.random.default_rng(9)
            P = torch.from_numpy(rng.uniform(v.min(0) - 0.3, v.max(0) + 0.3, (4000, 3)).astype(F32)).to(dev)
            far = before.squared_distance(P)[0] > (2 * h) ** 2
            w0, w1 = before.winding_number(P, math.inf), after.winding_number(P, math.inf)
            inside = (w0 > 0.5)[far]
            assert int(far.sum()) > 1000 and int(inside.sum()) > 100 and int((~inside).sum()) > 100
            assert torch.equal(inside, (w1 > 0.5)[far])
    # and it is the statement's pipeline, bit for bit: the winding numbers are integers to 1e-12, so the field has the same fp32 values
    import winding_statement as wn
    origin, dims, Pn = st.level_set_grid(v, h)
    S = (0.5 - wn.exact(Pn, v, f)[0]).astype(F32).reshape(dims)
    Vs, Es, Fs = st.extract(S, 0.0, origin, h)
    assert np.array_equal(v2.view(np.int32), Vs.view(np.int32)) and np.array_equal(f2, Fs)
    vn, fn = remesh_level_set(v, f, h, beta=math.inf)          # numpy in, numpy out
    assert isinstance(vn, np.ndarray) and np.array_equal(vn.view(np.int32), Vs.view(np.int32)) and np.array_equal(fn, Fs)


def test_signed_distance_field_and_offset(dev):
    """field='signed_distance' with a positive offset dilates. The distance d to the mesh is 1-Lipschitz, so along a grid edge of length
    l <= sqrt(3) h its linear interpolant is off by at most l (|d(x) - d(a)| <= t l and |lin(x) - d(a)| <= t l, the same from b): a vertex
    of the result has |d - offset| <= sqrt(3) h. The icosphere's faces lie within `dent` inside the unit sphere, dent = 1 - the smallest
    distance of a face's plane from the centre. So every vertex has |r - (1 + offset)| <= sqrt(3) h + dent, and with h = 0.1 and
    offset = 0.25 a result that was not dilated (r about 1) would miss that."""
    from largesteps import synthetic
    from largesteps.levelset import remesh_level_set
    v, f = synthetic.icosphere(8)
    f = np.asarray(f, dtype=np.int64)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    dent = 1.0 - np.abs(np.einsum("ij,ij->i", n / np.linalg.norm(n, axis=1, keepdims=True), a)).min()
    h, offset = 0.1, 0.25
    V2, F2 = remesh_level_set(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), h, field="signed_distance", offset=offset,
                              pad=4)                                   # pad * h must pass the offset, or the dilated surface leaves the grid
    v2, f2 = V2.cpu().numpy(), F2.cpu().numpy()
    r = np.linalg.norm(v2.astype(np.float64), axis=1)
    bound = math.sqrt(3.0) * h + dent
    print(f"dilated sphere: radius within {np.abs(r - 1.0 - offset).max():.4f} of {1 + offset}, bound {bound:.4f} (dent {dent:.4f})")
    assert bound < offset and np.abs(r - 1.0 - offset).max() <= bound
    assert st.boundary_edges(f2).shape[0] == 0 and st.euler(v2, f2) == 2 and st.signed_volume(v2, f2) > 0
