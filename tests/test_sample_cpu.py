"""
The surface sampler without a device: tests/sample_statement.py (the rule the device must match bit for bit) against known answers --
Philox4x32-10's published vectors, the counts of a mesh whose areas are exact, faces that must never be drawn, the slice law -- and
the boundary of largesteps.sampling and distance.chamfer_distance that answers before any device work: the C ABI's argument checks
and the Python-side errors.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import sample_statement as ss

F32 = np.float32
COUNTS = [1856, 3616, 5545, 7172, 8964, 10880, 12878, 14625]        # n = 65536, seed 0, stream 0 on triangles_with_bases()


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = ss.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert " ".join(f"{int(x):08x}" for x in got) == want
    # and vectorised: a row of a batch is the same call
    batch = ss.philox4x32_10(np.array([counter, (1, 2, 3, 4)], np.uint64), np.array(key, np.uint64))
    assert np.array_equal(batch[0], got)


def test_mulhi64_is_the_high_word():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.integers(0, 2 ** 64, 200, dtype=np.uint64), np.array([0, 1, 2 ** 64 - 1, 2 ** 32, 2 ** 32 - 1], np.uint64)])
    b = np.concatenate([rng.integers(0, 2 ** 64, 200, dtype=np.uint64), np.array([2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32, 2 ** 32 + 1], np.uint64)])
    assert [int(x) for x in ss.mulhi64(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]


def test_the_rule_on_exact_areas():
    v, f = ss.triangles_with_bases()
    assert np.array_equal(ss.areas(v, f), np.arange(1, 9) / 2.0)
    q, cumq, Q = ss.weights(v, f)
    assert [int(x) for x in q] == [k * 2 ** 29 for k in range(1, 9)] and Q == 36 * 2 ** 29
    n = 65536
    P, I, W = ss.sample_surface(v, f, n)
    counts = np.bincount(I, minlength=8)
    assert counts.tolist() == COUNTS
    prob = np.arange(1, 9) / 36.0
    z = (counts - n * prob) / np.sqrt(n * prob * (1 - prob))
    print("largest |z|:", float(np.abs(z).max()))
    assert (np.abs(z) < 5).all()
    # the point is the weights' combination, inside its face, and the weights are a partition of one to fp32 rounding
    assert P.dtype == F32 and W.dtype == F32 and I.dtype == np.int64
    assert (W >= 0).all() and np.abs(W.astype(np.float64).sum(1) - 1).max() <= 2.0 ** -23
    a, b, c = (v[f[I, k]].astype(np.float64) for k in range(3))
    Wd = W.astype(np.float64)
    assert np.array_equal(P, ((Wd[:, :1] * a + Wd[:, 1:2] * b) + Wd[:, 2:] * c).astype(F32))
    assert (P[:, 2] == 0).all() and (P[:, 1] >= 0).all() and (P[:, 1] <= 1).all()
    # sqrt-barycentric weights are uniform on the face: the mean point is the centroid
    for k in range(8):
        m = I == k
        centroid = v[f[k]].astype(np.float64).mean(0)
        assert np.abs(P[m].astype(np.float64).mean(0) - centroid).max() < 5 * (k + 1) / math.sqrt(18.0 * m.sum())


def test_faces_that_are_never_drawn():
    v, f = ss.triangles_with_bases([1, 2, 3])
    v = np.concatenate([v, [[9, 9, 9], [9, 9, 9], [np.nan, 0, 0]]]).astype(F32)
    # a zero-area face (three equal corners), a collinear one, one with a NaN corner, one with an index out of range
    f = np.concatenate([f[:1], [[9, 10, 9]], f[1:2], [[0, 1, 1]], [[0, 1, 11]], f[2:], [[0, 1, 99]]]).astype(np.int64)
    q, cumq, Q = ss.weights(v, f)
    assert (q[[1, 3, 4, 6]] == 0).all() and (q[[0, 2, 5]] > 0).all()
    P, I, W = ss.sample_surface(v, f, 20000, seed=3)
    assert set(np.unique(I).tolist()) == {0, 2, 5} and np.isfinite(P).all()
    # a face below amax 2^-32 quantises to 0
    v2, f2 = ss.triangles_with_bases([2.0 ** 33, 1, 1])
    assert [int(x) for x in ss.weights(v2, f2)[0]] == [2 ** 32, 0, 0]
    assert (ss.sample_surface(v2, f2, 1000)[1] == 0).all()


def test_no_face_can_be_drawn():
    v = np.zeros((4, 3), F32)
    for f in (np.zeros((0, 3), np.int64), np.array([[0, 1, 2], [1, 2, 3]]), np.array([[0, 1, 7]])):
        P, I, W = ss.sample_surface(v, f, 5)
        assert np.isnan(P).all() and (I == -1).all() and (W == 0).all() and P.shape == (5, 3) and W.shape == (5, 3)
    v[0, 0] = np.nan
    P, I, W = ss.sample_surface(v, np.array([[0, 1, 2]]), 5)
    assert np.isnan(P).all() and (I == -1).all() and (W == 0).all()


def test_slice_law_of_the_statement():
    v, f = ss.triangles_with_bases()
    P, I, W = ss.sample_surface(v, f, 1000, seed=2 ** 40 + 5, stream=7)
    P2, I2, W2 = ss.sample_surface(v, f, 200, seed=2 ** 40 + 5, stream=7, offset=300)
    assert np.array_equal(P[300:500], P2) and np.array_equal(I[300:500], I2) and np.array_equal(W[300:500], W2)
    # the counter's high word takes over at 2^32, and seed / stream select other sequences
    x = ss.words(4, offset=2 ** 32 - 2)
    assert np.array_equal(x[2], ss.philox4x32_10(np.array([0, 1, 0, 0], np.uint64), np.array([0, 0], np.uint64)))
    assert not np.array_equal(ss.words(4, seed=1), ss.words(4)) and not np.array_equal(ss.words(4, stream=1), ss.words(4))
    assert not np.array_equal(ss.words(4, seed=1 << 32), ss.words(4))


def test_gradient_statement_is_the_autograd_of_the_combination():
    v, f = ss.triangles_with_bases()
    f = np.concatenate([f, [[0, 4, 8]]])             # shared vertices: sums over several faces
    P, I, W = ss.sample_surface(v, f, 500, seed=1)
    gP = np.random.default_rng(0).normal(size=P.shape).astype(F32)
    V = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    tF, tI, tW = torch.from_numpy(f), torch.from_numpy(I), torch.from_numpy(W).double()
    out = sum(tW[:, k, None] * V[tF[tI, k]] for k in range(3))
    (out * torch.from_numpy(gP).double()).sum().backward()
    g, mag = ss.grad_vertices(v, f, I, W, gP)
    assert (np.abs(g - V.grad.numpy()) <= 2.0 ** -40 * mag).all() and (mag >= np.abs(g)).all()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks():
    from largesteps import _native
    lib = _native.lib()
    n = ctypes.c_size_t(0)
    assert lib.ls_sample_workspace_bytes(1000, 1000, ctypes.byref(n)) == 0
    # forward: two scalars, F words, a word per tile; backward: keys, order, segments, the sort's scratch and 9 fp64 per face
    assert n.value >= max(16 + 8 * 1000 + 8 * 2, 4 * 1000 * 2 + 4 * 1002 + 72 * 1000)
    assert lib.ls_sample_workspace_bytes(0, 0, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.ls_sample_workspace_bytes(-1, 1, ctypes.byref(n)) == _native.LS_E_INVALID
    assert lib.ls_sample_workspace_bytes(1, -1, ctypes.byref(n)) == _native.LS_E_INVALID
    assert lib.ls_sample_workspace_bytes(1, 1, None) == _native.LS_E_INVALID
    assert lib.ls_sample_workspace_bytes(2 ** 31, 1, ctypes.byref(n)) == _native.LS_E_OVERFLOW
    assert lib.ls_sample_workspace_bytes(1, 2 ** 31, ctypes.byref(n)) == _native.LS_E_OVERFLOW
    one = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any device work
    assert lib.ls_sample_surface(one, one, 2, 1, 3, 1, 0, 0, 0, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert "int32 or int64" in _native.last_error()
    assert lib.ls_sample_surface(None, one, 4, 1, 3, 1, 0, 0, 0, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert lib.ls_sample_surface(one, one, 4, 1, 3, 1, 0, 0, 0, None, one, one, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert lib.ls_sample_surface(one, one, 4, 1, 3, -1, 0, 0, 0, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert lib.ls_sample_surface(one, one, 4, 1, 3, 2 ** 31, 0, 0, 0, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_OVERFLOW
    assert lib.ls_sample_surface(one, one, 4, 2 ** 31, 3, 1, 0, 0, 0, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_OVERFLOW
    assert lib.ls_sample_surface(one, one, 4, 1, 3, 1, 0, 0, 2 ** 31 - 1, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_OVERFLOW
    assert lib.ls_sample_surface(one, one, 4, 1, 3, 1, 0, 0, 0, one, one, one, one, 8, 0, None) == _native.LS_E_WORKSPACE
    assert lib.ls_sample_surface_backward(one, 4, 1, 3, 1, one, one, one, one, one, None, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert lib.ls_sample_surface_backward(one, 4, 1, 0, 1, one, one, one, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_INVALID
    assert lib.ls_sample_surface_backward(one, 4, 1, 3, 2 ** 31, one, one, one, one, one, one, one, 1 << 20, 0, None) == _native.LS_E_OVERFLOW
    assert lib.ls_sample_surface_backward(one, 4, 1, 3, 1, one, one, one, one, one, one, one, 8, 0, None) == _native.LS_E_WORKSPACE


def test_scan_tile_is_the_headers():
    import os
    import re
    from largesteps import sampling
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "largesteps_hip.h")).read()
    assert int(re.search(r"#define LS_SAMPLE_SCAN_TILE (\d+)", header).group(1)) == sampling.SCAN_TILE


def test_sample_surface_refuses_before_any_device_work():
    from largesteps.sampling import sample_surface
    v, f = ss.triangles_with_bases()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError, match="HIP device"):
        sample_surface(tv, tf, 4)                                   # CPU tensors
    with pytest.raises(TypeError):
        sample_surface(v, f.astype(np.float32), 4)
    with pytest.raises(TypeError):
        sample_surface(v.astype(complex), f, 4)
    with pytest.raises(ValueError):
        sample_surface(v[:, :2], f, 4)
    with pytest.raises(ValueError):
        sample_surface(v, f[:, :2], 4)
    with pytest.raises(ValueError):
        sample_surface(v, f.reshape(-1), 4)
    with pytest.raises(ValueError):
        sample_surface(v, f, -1)
    with pytest.raises(TypeError):
        sample_surface(v, f, 4.0)
    with pytest.raises(TypeError):
        sample_surface(v, f, 4, seed=1.5)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(stream=-1), dict(stream=2 ** 32), dict(offset=-1)):
        with pytest.raises(ValueError):
            sample_surface(v, f, 4, **kw)
    with pytest.raises(OverflowError):
        sample_surface(v, f, 2 ** 31)
    with pytest.raises(OverflowError):
        sample_surface(v, f, 1, offset=2 ** 31 - 1)
    with pytest.raises(OverflowError):
        sample_surface(v, f, 2 ** 30, offset=2 ** 30)


def test_chamfer_distance_refuses_before_any_device_work():
    from largesteps.distance import chamfer_distance
    v, f = ss.triangles_with_bases()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError, match="HIP device"):
        chamfer_distance(tv, tf, tv, tf, 16)
    with pytest.raises(TypeError):
        chamfer_distance(v, f.astype(np.float64), v, f, 16)
    with pytest.raises(TypeError):
        chamfer_distance(v, f, v.astype(complex), f, 16)
    with pytest.raises(ValueError):
        chamfer_distance(v, f, v[:, :2], f, 16)
    with pytest.raises(ValueError):
        chamfer_distance(v, f[:, :2], v, f, 16)
    for n in (0, -3):
        with pytest.raises(ValueError):
            chamfer_distance(v, f, v, f, n)
    with pytest.raises(TypeError):
        chamfer_distance(v, f, v, f, 16.0)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            chamfer_distance(v, f, v, f, 16, seed=seed)
    with pytest.raises(TypeError):
        chamfer_distance(v, f, v, f, 16, seed="0")
