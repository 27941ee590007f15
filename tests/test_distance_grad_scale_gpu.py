"""
The gradient of largesteps.distance to the mesh vertices on the device (csrc/distance.hip) at the cases of tests/distance_grad_cases.py:
several sort workgroups, one, two and three byte passes, both switches of the sort's chunk, per-face counts on either side of 64 at
every place of a wave, a vertex with 1200 corners, face ids outside [0, F). For every case (U = 2^-24):
  gP   |err| <= 16 U |term|, the points with an id outside [0, F) included;
  gV   |err| <= (chain + 16) U sum |terms| against the fp64 sums of tests/distance_grad_statement.py, and THE BITS of its
       `ordered_gradients`, the fp32 sums in the stated order: what tells that order from any other;
  the workspace is exactly ls_mesh_distance_backward_workspace_bytes inside a larger buffer, and the 4096 bytes on either side of it still
  hold their pattern afterwards.
"""
import ctypes

import numpy as np
import pytest
import torch

import distance_grad_cases as dc
import distance_grad_statement as dg
from test_distance_grad_gpu import bits

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GUARD, PATTERN = 4096, 0xA5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def handle(dev, v, f, idx=np.int64):
    from largesteps.distance import MeshDistance
    return MeshDistance(*to(dev, v, f.astype(idx)))


def device_weights(dev, m, P, I):
    from largesteps import _native
    W = torch.empty((P.shape[0], 3), dtype=torch.float64, device=dev)
    _native.check(_native.lib().ls_mesh_distance_weights(m._h, _native.ptr(P), P.shape[0], _native.ptr(I), _native.ptr(W), _native.stream_of(dev)))
    return W.cpu().numpy()


def backward(dev, m, P, I, C, G):
    """ls_mesh_distance_backward on device tensors -> (gP, gV) tensors. The outputs start as NaN, so an entry the call leaves alone shows;
    the workspace has exactly the stated size and sits between two guard bands"""
    from largesteps import _native
    lib, n = _native.lib(), P.shape[0]
    vptr, order = m._corner_ranks()
    need = ctypes.c_size_t(0)
    _native.check(lib.ls_mesh_distance_backward_workspace_bytes(n, m._f.shape[0], ctypes.byref(need)))
    buf = torch.full((need.value + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + need.value]
    assert ws.data_ptr() % 8 == 0
    gP = torch.full_like(P, float("nan"))
    gV = torch.full_like(m.V, float("nan"))
    args = (m._h, _native.ptr(P), n, _native.ptr(I), _native.ptr(C), _native.ptr(G), _native.ptr(vptr), _native.ptr(order), _native.ptr(gP),
            _native.ptr(gV), _native.ptr(ws))
    with torch.cuda.device(dev):
        assert lib.ls_mesh_distance_backward(*args, need.value - 1, _native.stream_of(dev)) == _native.LS_E_WORKSPACE
        _native.check(lib.ls_mesh_distance_backward(*args, need.value, _native.stream_of(dev)))
    torch.cuda.synchronize(dev)
    assert bool((buf[:GUARD] == PATTERN).all()), "the workspace was written below its start"
    assert bool((buf[GUARD + need.value:] == PATTERN).all()), "the workspace was written past its stated size"
    return gP, gV


def check(name, m, v, f, P, I, C, g, gP, gV):
    """the assertions of the module docstring on numpy inputs and the device's (gP, gV) tensors; returns gV's bits"""
    vptr, order = (x.cpu().numpy() for x in m._corner_ranks())
    assert gP.dtype == torch.float32 and gV.dtype == torch.float32 and gP.shape == P.shape and gV.shape == v.shape
    gP, gV = gP.cpu().numpy(), gV.cpu().numpy()
    assert np.isfinite(gP).all() and np.isfinite(gV).all()
    ok = (I >= 0) & (I < f.shape[0])
    t = dg.terms(P[ok], v, f, I[ok], C[ok], g[ok])
    want = dg.gradients(P[ok], v, f, I[ok], C[ok], g[ok], t=t)
    tP = dg.point_terms(P, C, g).astype(np.float64)
    assert np.array_equal(tP[ok], want["gP"].astype(np.float64))
    err = np.abs(gP.astype(np.float64) - tP)
    print(f"{name}: {len(I)} points ({int((~ok).sum())} outside), {f.shape[0]} faces; gP: largest error / |term| "
          f"{float((err / np.maximum(np.abs(tP), 1e-300)).max()):.3e}")
    assert (err <= 16 * U * np.abs(tP)).all()
    err = np.abs(gV.astype(np.float64) - want["gV"])
    bound = (want["depth"][:, None] + 16) * U * want["abs"]
    nz = want["abs"] > 0
    print(f"{name}: gV: largest error / bound {float((err[nz] / bound[nz]).max()):.3e}, deepest chain {int(want['depth'].max())}, "
          f"most points on a face {int(np.bincount(I[ok], minlength=1).max())}")
    assert (err <= bound).all()
    touched = np.zeros(v.shape[0], dtype=bool)
    touched[f[I[ok]].reshape(-1)] = True
    assert not gV[~touched].any()
    exact = dg.ordered_gradients(P, v, f, I, C, g, vptr, order, t=t)
    differ = (gV.view(np.int32) != exact.view(np.int32)).any(1)
    assert not differ.any(), f"{int(differ.sum())} of {v.shape[0]} vertex rows differ from the ordered sums, first {np.nonzero(differ)[0][:4].tolist()}"
    return gV.view(np.int32)


@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_walked_three_pass(dev, idx):
    """the device's own I and C through autograd: three byte passes over 34 sort workgroups; the weights and the raw call give the same
    bits, as do a second run and a captured forward and backward"""
    v, f, p = dc.walked_three_pass()
    g = np.random.default_rng(58).uniform(-1.0, 2.0, p.shape[0])
    V, P = (x.requires_grad_() for x in to(dev, v, p))
    G, = to(dev, g)
    from largesteps.distance import MeshDistance
    with MeshDistance(V, to(dev, f.astype(idx))[0]) as m:
        def step():
            d2, I, C = m.squared_distance(P)
            gP, gV = torch.autograd.grad((d2 * G).sum(), (P, V))
            return d2.detach(), I, C, gP, gV
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            eager = [x.clone() for x in step()]                  # the warm-up: builds the corner ranking
        torch.cuda.current_stream(dev).wait_stream(s)
        _, tI, tC, gP, gV = eager
        I, C = tI.cpu().numpy(), tC.cpu().numpy()
        got_w, want_w = device_weights(dev, m, P.detach(), tI), dg.weights(p, v, f, I)
        assert np.array_equal(got_w.view(np.int64), want_w.view(np.int64)), f"{int((got_w != want_w).any(1).sum())} weight rows differ"
        raw = backward(dev, m, P.detach(), tI, tC, G)
        assert torch.equal(bits(raw[0]), bits(gP)) and torch.equal(bits(raw[1]), bits(gV))
        for a, b in zip(eager, step()):
            assert torch.equal(bits(a), bits(b))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        for a, b in zip(eager, out):
            assert torch.equal(bits(a), bits(b))
        check("walked_three_pass", m, v, f, p, I, C, g, gP, gV)


def run_fabricated(dev, name, case=None):
    v, f, P, I, C, g = case if case is not None else dc.fabricated(name)
    with handle(dev, v, f) as m:
        gP, gV = backward(dev, m, *to(dev, P, I, C, g))
        return check(name, m, v, f, P, I, C, g, gP, gV)


@pytest.mark.parametrize("name", ["one_pass_many_blocks", "thresholds", "hub"])
def test_fabricated(dev, name):
    run_fabricated(dev, name)


def test_out_of_range(dev):
    """ids -1, T, T + 1 and 2^40 on one point in a hundred: those points get their gP, NaN weights from the bare weights call, and add
    nothing to gV, which has the bits of the call without them"""
    v, f, P, I, C, g = dc.fabricated("out_of_range")
    T = f.shape[0]
    bad = (I < 0) | (I >= T)
    assert bad.any() and set(I[bad].tolist()) == set(dc.out_of_range_ids(T).tolist())
    with_them = run_fabricated(dev, "out_of_range", (v, f, P, I, C, g))
    without = run_fabricated(dev, "out_of_range without them", (v, f, P[~bad], I[~bad], C[~bad], g[~bad]))
    assert np.array_equal(with_them, without)
    with handle(dev, v, f) as m:
        tP, = to(dev, P)
        W = device_weights(dev, m, tP, to(dev, I)[0])
        W_in_range = device_weights(dev, m, tP, to(dev, dc.fabricated_ids("thresholds"))[0])
    assert np.isnan(W[bad]).all() and np.isfinite(W[~bad]).all()
    assert np.array_equal(W[~bad].view(np.int64), W_in_range[~bad].view(np.int64))
    assert np.array_equal(W[~bad].view(np.int64), dg.weights(P[~bad], v, f, I[~bad]).view(np.int64))


@pytest.mark.parametrize("name", list(dc.CHUNK_N))
def test_chunks(dev, name):
    """the last n with 1024 points a sort workgroup, the first with 2048 and the first with 4096, on 67 280 faces"""
    run_fabricated(dev, name)
