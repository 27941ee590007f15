"""
largesteps.sampling on the device (csrc/sample.hip) against tests/sample_statement.py: P, I and W bit for bit -- around the wave, the
scan's tile and past it, at the sample counts around a workgroup, for both index types, every argument of the sequence and input that
is not contiguous or not aligned --, the known counts, degenerate input, the slice law, the gradient to V against its fp64 value,
a captured forward and backward, and distance.chamfer_distance built on it.
"""
import numpy as np
import pytest
import torch

import distance_statement as ds
import sample_statement as ss
from largesteps import synthetic
from test_sample_cpu import COUNTS

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = 2048


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def fan(F):
    """F triangles around vertex 0, the rim at radii 1 .. 7 and slightly off the plane: areas between about 0.02 and 1 of the largest"""
    t = 2.0 * np.pi * np.arange(F + 1) / (F + 1)
    r = 1.0 + (np.arange(F + 1) % 7)
    rim = np.stack([r * np.cos(t), r * np.sin(t), 0.1 * np.sin(5 * t)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.3]], rim]).astype(F32)
    f = np.stack([np.zeros(F, np.int64), np.arange(1, F + 1), np.arange(2, F + 2)], 1)
    return v, f


_meshes = {}


def mesh(name):
    if name not in _meshes:
        kind, size = name.split("-")
        if kind == "fan":
            _meshes[name] = fan(int(size))
        elif kind == "ico":
            v, f = synthetic.icosphere(int(size))
            _meshes[name] = (synthetic.perturb(v, radial=0.05, seed=1).astype(F32), f)
        else:
            _meshes[name] = synthetic.plane(int(size))
    return _meshes[name]


def test_the_cases_stand_where_the_kernels_change_path():
    from largesteps import sampling
    assert sampling.SCAN_TILE == TILE
    assert mesh("plane-33")[1].shape[0] == TILE and mesh("plane-400")[1].shape[0] == 318402 > 2 * TILE


def bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    return x.view(np.int32) if x.dtype == np.float32 else x


def device_sample(dev, v, f, n, idx=np.int64, **kw):
    from largesteps.sampling import sample_surface
    out = sample_surface(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(f).astype(idx)).to(dev), n, **kw)
    assert out[0].dtype == torch.float32 and out[0].shape == (n, 3) and out[1].dtype == torch.int64 and out[1].shape == (n,)
    assert out[2].dtype == torch.float32 and out[2].shape == (n, 3)
    return out


def same(got, want):
    for g, w, what in zip(got, want, "PIW"):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = bits(g) != bits(w)
        assert not bad.any(), f"{what}: {int(bad.reshape(len(g), -1).any(1).sum())} of {len(g)} rows differ, first at {int(np.argwhere(bad)[0][0])}"


SIZES = ["fan-1", "fan-2", "fan-63", "fan-64", "fan-65", f"fan-{TILE - 1}", f"fan-{TILE}", f"fan-{TILE + 1}", "plane-5", "plane-33", "plane-34"]


@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 16 + 1])
@pytest.mark.parametrize("name", SIZES)
def test_samples_are_the_statement_bitwise(dev, name, n):
    v, f = mesh(name)
    same(device_sample(dev, v, f, n, np.int32 if n in (255, 2 ** 16 + 1) else np.int64), ss.sample_surface(v, f, n))


@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_past_one_tile_of_the_scan(dev, idx):
    v, f = mesh("plane-400")                       # 156 tiles: every tile but the first adds the scanned sum of those before it
    n = 2 ** 16 + 1
    got = device_sample(dev, v, f, n, idx)
    same(got, ss.sample_surface(v, f, n))
    assert int(got[1].max()) > 300000 and int(got[1].min()) < 2000


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("kw", [dict(seed=1), dict(seed=2 ** 64 - 1), dict(seed=2 ** 32), dict(stream=1), dict(stream=2 ** 32 - 1), dict(offset=1),
                                dict(offset=2 ** 31 - 1 - 257), dict(seed=0x9E3779B97F4A7C15, stream=12345, offset=2 ** 20 + 3)],
                         ids=lambda kw: ",".join(f"{k}={v:#x}" for k, v in kw.items()))
def test_seed_stream_and_offset(dev, kw, idx):
    v, f = mesh("fan-65")
    same(device_sample(dev, v, f, 257, idx, **kw), ss.sample_surface(v, f, 257, **kw))


def test_input_that_is_not_contiguous_or_not_aligned(dev):
    from largesteps.sampling import sample_surface
    v, f = mesh("plane-34")
    want = ss.sample_surface(v, f, 257, seed=5)
    wide = torch.zeros((v.shape[0], 4), dtype=torch.float32, device=dev)
    wide[:, :3] = torch.from_numpy(v).to(dev)
    ft = torch.from_numpy(np.ascontiguousarray(f.T)).to(dev).t()              # (F, 3) with strides (1, F)
    assert not wide[:, :3].is_contiguous() and not ft.is_contiguous()
    same(sample_surface(wide[:, :3], ft, 257, seed=5), want)
    for idx in (torch.int32, torch.int64):
        flat = torch.zeros(3 * v.shape[0] + 1, dtype=torch.float32, device=dev)
        flat[1:] = torch.from_numpy(v).to(dev).reshape(-1)
        fflat = torch.zeros(3 * f.shape[0] + 1, dtype=idx, device=dev)
        fflat[1:] = torch.from_numpy(f).to(dev).reshape(-1).to(idx)
        V1, F1 = flat[1:].view(-1, 3), fflat[1:].view(-1, 3)
        assert V1.data_ptr() % 16 == 4 and F1.data_ptr() % 16 == fflat.element_size()
        same(sample_surface(V1, F1, 257, seed=5), want)
    # numpy in, numpy out, on the current device; float64 positions are converted
    got = sample_surface(v.astype(np.float64), f.astype(np.int32), 257, seed=5)
    assert all(isinstance(x, np.ndarray) for x in got)
    same(got, want)


def test_known_counts_on_the_device(dev):
    v, f = ss.triangles_with_bases()
    _, I, _ = device_sample(dev, v, f, 65536)
    assert torch.bincount(I, minlength=8).tolist() == COUNTS


def test_one_face_outweighs_the_rest(dev):
    """a face 2^40 times the others: they quantise to 0 and are never drawn"""
    v, f = ss.triangles_with_bases([1, 1, 1])                                   # areas 2^-1 ...
    v = np.concatenate([v, [[0, 0, 0], [2.0 ** 20, 0, 0], [0, 2.0 ** 20, 0]]]).astype(F32)
    f = np.concatenate([f[:1], [[9, 10, 11]], f[1:]])                           # ... and 2^39, as face 1
    assert np.array_equal(ss.areas(v, f), [0.5, 2.0 ** 39, 0.5, 0.5]) and [int(x) for x in ss.weights(v, f)[0]] == [0, 2 ** 32, 0, 0]
    got = device_sample(dev, v, f, 4097)
    same(got, ss.sample_surface(v, f, 4097))
    assert bool((got[1] == 1).all())
    v[10, 0] = v[11, 1] = F32(2.0 ** 16)                                        # 2^32 times larger: the small faces have q = 1
    assert [int(x) for x in ss.weights(v, f)[0]] == [1, 2 ** 32, 1, 1]
    same(device_sample(dev, v, f, 4097), ss.sample_surface(v, f, 4097))


def test_faces_that_are_never_drawn_on_the_device(dev):
    v, f = ss.triangles_with_bases([1, 2, 3])
    v = np.concatenate([v, [[9, 9, 9], [9, 9, 9], [np.nan, 0, 0]]]).astype(F32)
    f = np.concatenate([f[:1], [[9, 10, 9]], f[1:2], [[0, 1, 1]], [[0, 1, 11]], f[2:], [[0, 1, 99]], [[-1, 1, 2]]]).astype(np.int64)
    for idx in (np.int32, np.int64):
        got = device_sample(dev, v, f, 4097, idx, seed=3)         # (no gradient asked: nothing ranks the corners, nothing raises)
        same(got, ss.sample_surface(v, f, 4097, seed=3))
        assert set(torch.unique(got[1]).tolist()) == {0, 2, 5}


@pytest.mark.parametrize("case", ["zero areas", "nan", "no faces", "out of range"])
def test_no_face_can_be_drawn(dev, case):
    v = np.zeros((4, 3), F32)
    f = np.array([[0, 1, 2], [1, 2, 3]])
    if case == "nan":
        v[:] = np.nan
    elif case == "no faces":
        f = np.zeros((0, 3), np.int64)
    elif case == "out of range":
        v[:] = np.arange(12).reshape(4, 3) ** 2
        f = f + 2
    P, I, W = device_sample(dev, v, f, 300)
    assert bool(torch.isnan(P).all()) and bool((I == -1).all()) and not bool(W.any())
    same((P, I, W), ss.sample_surface(v, f, 300))           # (one NaN: the quiet one with an empty payload)
    assert device_sample(dev, v, f, 0)[0].shape == (0, 3)


def test_slice_law(dev):
    v, f = mesh("ico-3")
    for idx in (np.int32, np.int64):
        whole = device_sample(dev, v, f, 1000, idx, seed=9, stream=2)
        part = device_sample(dev, v, f, 200, idx, seed=9, stream=2, offset=300)
        for a, b in zip(whole, part):
            assert np.array_equal(bits(a[300:500]), bits(b))
        again = device_sample(dev, v, f, 1000, idx, seed=9, stream=2)
        for a, b in zip(whole, again):
            assert np.array_equal(bits(a), bits(b))


# ---- gradient --------------------------------------------------------------------------------------------------------------------
def with_spare_parts(v, f):
    """the mesh plus a zero-area face on three vertices of its own and a vertex no face names: no sample touches them"""
    nv = v.shape[0]
    v = np.concatenate([v, np.full((3, 3), 2.0, F32), [[5.0, 5.0, 5.0]]]).astype(F32)
    return v, np.concatenate([f, [[nv, nv + 1, nv + 2]]])


def grad_run(dev, v, f, n, gP, idx=np.int64, **kw):
    from largesteps.sampling import sample_surface
    V = torch.from_numpy(v).to(dev).requires_grad_()
    P, I, W = sample_surface(V, torch.from_numpy(f.astype(idx)).to(dev), n, **kw)
    assert P.requires_grad and not I.requires_grad and not W.requires_grad
    P.backward(torch.from_numpy(gP).to(dev))
    return P.detach(), I, W, V.grad


# (mesh, n, some face is summed by a whole wave, some face by one thread): fan-65 has a vertex with 65 corners and areas 1 : 21 apart
@pytest.mark.parametrize("name, n, long, short", [("ico-4", 2 ** 16, True, False), ("plane-9", 2 ** 14, True, False), ("fan-65", 4096, True, True),
                                                  ("fan-65", 100, False, True), ("plane-34", 2 ** 16 + 1, False, True)])
def test_gradient_to_the_vertices(dev, name, n, long, short):
    v, f = with_spare_parts(*mesh(name))
    gP = np.random.default_rng(len(name) + n).uniform(-1.0, 2.0, (n, 3)).astype(F32)
    P, I, W, gV = grad_run(dev, v, f, n, gP, seed=4)
    assert gV.dtype == torch.float32 and gV.shape == v.shape
    same((P, I, W), ss.sample_surface(v, f, n, seed=4))                   # the differentiable path returns the plain path's bits
    I, W = I.cpu().numpy(), W.cpu().numpy()
    counts = np.bincount(I, minlength=f.shape[0])
    valence = np.bincount(f.reshape(-1), minlength=v.shape[0])
    print(f"{name}: samples per face {counts.min()} .. {counts.max()}, largest valence {valence.max()}")
    assert (counts.max() > 64) == long and (counts[counts > 0].min() <= 64) == short, "the case does not reach the path it is here for"
    # the reference: fp64 autograd of sum_k W[:, k, None] * V[F[I, k]] with the I and W the forward returned
    Vd = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    tF, tI, tW = torch.from_numpy(f), torch.from_numpy(I), torch.from_numpy(W).double()
    (sum(tW[:, k, None] * Vd[tF[tI, k]] for k in range(3)) * torch.from_numpy(gP).double()).sum().backward()
    want = Vd.grad.numpy()
    mag = ss.grad_vertices(v, f, I, W, gP)[1]
    got = gV.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    bound = np.spacing(np.abs(want).astype(F32)).astype(np.float64) + 2.0 ** -40 * mag
    print(f"largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    # a vertex that no sample touches gets exact zeros (+0.0)
    touched = np.zeros(v.shape[0], dtype=bool)
    touched[f[I].reshape(-1)] = True
    assert not touched[-4:].any() and (~touched).sum() >= 4
    assert not bits(got[~touched]).any()
    # two runs, and the other index type, give the same bits
    for idx in (np.int64, np.int32):
        assert np.array_equal(bits(grad_run(dev, v, f, n, gP, idx, seed=4)[3]), bits(got))


def test_gradient_of_nothing(dev):
    v, f = mesh("fan-65")
    gV = grad_run(dev, v, f, 0, np.zeros((0, 3), F32))[3]
    assert gV.shape == v.shape and not bits(gV).any()
    z = np.zeros_like(v)                            # no face can be drawn: I = -1 adds nothing
    gV = grad_run(dev, z, f, 500, np.ones((500, 3), F32))[3]
    assert not bits(gV).any()


def test_a_bad_index_raises_where_the_corners_are_ranked(dev):
    from largesteps.sampling import sample_surface
    v, f = mesh("fan-2")
    bad = f.copy()
    bad[1, 2] = v.shape[0]
    with pytest.raises(IndexError):
        sample_surface(torch.from_numpy(v).to(dev).requires_grad_(), torch.from_numpy(bad).to(dev), 8)


def test_a_captured_forward_and_backward_replays_bitwise(dev):
    from largesteps.sampling import sample_surface
    v, f = mesh("ico-4")
    n = 2 ** 14
    V = torch.from_numpy(v).to(dev).requires_grad_()
    tf = torch.from_numpy(f).to(dev)
    G = torch.from_numpy(np.random.default_rng(0).normal(size=(n, 3)).astype(F32)).to(dev)

    def step():
        P, I, W = sample_surface(V, tf, n, seed=11, stream=3, offset=17)
        gV, = torch.autograd.grad((P * G).sum(), (V,))
        return P.detach(), I, W, gV
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        eager = [x.clone() for x in step()]                  # the warm-up: builds the corner ranking
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for x in out:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    same(eager[:3], ss.sample_surface(v, f, n, seed=11, stream=3, offset=17))
    for a, b in zip(eager, out):
        assert np.array_equal(bits(a), bits(b))


# ---- chamfer_distance ------------------------------------------------------------------------------------------------------------
def chamfer_meshes():
    va, fa = synthetic.icosphere(3)                                            # 180 faces
    vb, fb = synthetic.icosphere(2)                                            # 80 faces
    vb = (synthetic.perturb(vb, radial=0.1, seed=2) * 1.1 + 0.05).astype(F32)
    return va, fa, vb, fb


def test_chamfer_distance_is_the_statement(dev):
    from largesteps.distance import MeshDistance, chamfer_distance
    from largesteps.sampling import sample_surface
    va, fa, vb, fb = chamfer_meshes()
    n, seed = 4096, 6
    tva, tfa, tvb, tfb = (torch.from_numpy(x).to(dev) for x in (va, fa, vb, fb))
    got = chamfer_distance(tva, tfa, tvb, tfb, n, seed=seed)
    assert got.dtype == torch.float64 and got.shape == () and got.device.type == "cuda" and not got.requires_grad
    pa, pb = ss.sample_surface(va, fa, n, seed=seed, stream=0)[0], ss.sample_surface(vb, fb, n, seed=seed, stream=1)[0]
    want = float(np.mean(ds.squared_distance(pa, vb, fb)[0]) + np.mean(ds.squared_distance(pb, va, fa)[0]))
    print(f"chamfer {float(got):.17g}, statement {want:.17g}, relative difference {abs(float(got) - want) / want:.3e}")
    assert want > 1e-3 and abs(float(got) - want) <= 1e-12 * want
    # its own two halves by hand, bit for bit
    with MeshDistance(tva, tfa) as a, MeshDistance(tvb, tfb) as b:
        PA, PB = sample_surface(tva, tfa, n, seed=seed, stream=0)[0], sample_surface(tvb, tfb, n, seed=seed, stream=1)[0]
        hand = b.squared_distance(PA)[0].mean() + a.squared_distance(PB)[0].mean()
    assert float(hand) == float(got)
    # numpy input: a float, the same value
    as_np = chamfer_distance(va, fa, vb, fb, n, seed=seed)
    assert isinstance(as_np, float) and as_np == float(got)
    assert chamfer_distance(tva, tfa, tvb, tfb, n, seed=seed + 1) != got


def test_chamfer_distance_gradient(dev):
    from largesteps.distance import chamfer_distance
    va, fa, vb, fb = chamfer_meshes()
    tfa, tfb = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev)

    def run():
        VA, VB = torch.from_numpy(va).to(dev).requires_grad_(), torch.from_numpy(vb).to(dev).requires_grad_()
        d = chamfer_distance(VA, tfa, VB, tfb, 4096, seed=1)
        assert d.requires_grad
        d.backward()
        return d.detach(), VA.grad, VB.grad
    first, again = run(), run()
    for g in first[1:]:
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                           b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
    # both paths reach VA: through A's samples (measured against B) and through A's faces closest to B's samples
    from largesteps.distance import MeshDistance
    from largesteps.sampling import sample_surface
    VA, VB = torch.from_numpy(va).to(dev).requires_grad_(), torch.from_numpy(vb).to(dev)
    with MeshDistance(VB, tfb) as b:
        through_samples, = torch.autograd.grad(b.squared_distance(sample_surface(VA, tfa, 4096, seed=1, stream=0)[0])[0].mean(), VA)
    with MeshDistance(VA, tfa) as a:
        through_faces, = torch.autograd.grad(a.squared_distance(sample_surface(VB, tfb, 4096, seed=1, stream=1)[0])[0].mean(), VA)
    assert bool(through_samples.abs().max() > 0) and bool(through_faces.abs().max() > 0)
    assert torch.equal(through_samples + through_faces, first[1])
    # a short descent on A lowers the value
    VA = torch.from_numpy(va).to(dev).requires_grad_()
    VB = torch.from_numpy(vb).to(dev)
    before = float(chamfer_distance(VA, tfa, VB, tfb, 4096, seed=1).detach())
    for it in range(5):
        VA.grad = None
        chamfer_distance(VA, tfa, VB, tfb, 4096, seed=1).backward()
        with torch.no_grad():
            VA -= 0.25 * VA.grad * VA.shape[0] / 6
    after = float(chamfer_distance(VA, tfa, VB, tfb, 4096, seed=1).detach())
    print(f"chamfer before {before:.6f}, after five steps {after:.6f}")
    assert after < before


def test_chamfer_distance_of_a_mesh_to_itself_is_small(dev):
    """Every sample is a point of one of the mesh's own faces up to the fp32 rounding of its three coordinates (half an ulp each; the
    coordinates of the unit sphere are at most 1, so 2^-25), and its distance to the mesh is at most its distance to that face: at
    most sqrt(3) 2^-25, eight orders of magnitude below an edge. The value is therefore of the order of 6 * 2^-50, and must lie below
    (mean edge length)^2."""
    from largesteps.distance import chamfer_distance
    va, fa, _, _ = chamfer_meshes()
    e = np.concatenate([va[fa[:, k]] - va[fa[:, (k + 1) % 3]] for k in range(3)]).astype(np.float64)
    mean_edge = float(np.sqrt((e * e).sum(1)).mean())
    tva, tfa = torch.from_numpy(va).to(dev), torch.from_numpy(fa).to(dev)
    d = float(chamfer_distance(tva, tfa, tva, tfa, 4096, seed=3))
    print(f"self chamfer {d:.3e}, (mean edge)^2 {mean_edge ** 2:.3e}")
    assert 0.0 <= d < mean_edge ** 2
