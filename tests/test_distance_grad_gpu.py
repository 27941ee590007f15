"""
The gradient of largesteps.distance on the device (csrc/distance.hip) against tests/distance_grad_statement.py: the weights bit for
bit, both gradients within the bound of the kernel's fp32 chain, reproducible across runs, streams and a captured graph; a mesh moved
under a live handle; the plain path untouched when nothing requires grad; and a short two-sided fit that uses all of it.
"""
import ctypes

import numpy as np
import pytest
import torch

import distance_grad_statement as dg
from test_distance_gpu import SMALL, mesh, probes
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32
N = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_cases = {}


def case(name, dev):
    """a SMALL mesh, its probes, the device's query and incoming gradients g, computed once: numpy (v, f, p, I, C, g)"""
    from largesteps.distance import MeshDistance
    if name not in _cases:
        v, f = mesh(name)
        f = np.asarray(f, dtype=np.int64)
        p = probes(v, f, N, seed=len(name))
        with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) as m:
            _, I, C = m.squared_distance(torch.from_numpy(p).to(dev))
        g = np.random.default_rng(len(name)).uniform(-1.0, 2.0, p.shape[0])
        _cases[name] = (v, f, p, I.cpu().numpy(), C.cpu().numpy(), g)
    return _cases[name]


def bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def run(dev, v, f, p, g, idx=np.int64, need_p=True, need_v=True, handle=None):
    """forward and backward through the public interface: (sqrD, I, C, gP, gV) tensors"""
    from largesteps.distance import MeshDistance
    P = torch.from_numpy(p).to(dev).requires_grad_(need_p)
    V = torch.from_numpy(v).to(dev).requires_grad_(need_v)
    m = handle if handle is not None else MeshDistance(V, torch.from_numpy(np.asarray(f).astype(idx)).to(dev))
    try:
        if handle is not None:
            m.update(V)
        d2, I, C = m.squared_distance(P)
        assert d2.requires_grad and d2.dtype == torch.float64 and not I.requires_grad and not C.requires_grad
        (d2 * torch.from_numpy(g).to(dev)).sum().backward()
    finally:
        if handle is None:
            m.close()
    return d2.detach(), I, C, P.grad, V.grad


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("name", SMALL)
def test_weights_are_the_statement_bitwise(dev, name, idx):
    from largesteps import _native
    from largesteps.distance import MeshDistance
    v, f, p, I, C, _ = case(name, dev)
    P, tI = torch.from_numpy(p).to(dev), torch.from_numpy(I).to(dev)
    W = torch.empty((p.shape[0], 3), dtype=torch.float64, device=dev)
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(idx)).to(dev)) as m:
        _native.check(_native.lib().ls_mesh_distance_weights(m._h, _native.ptr(P), p.shape[0], _native.ptr(tI), _native.ptr(W), _native.stream_of(dev)))
        got = W.cpu().numpy()
    want = dg.weights(p, v, f, I)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), f"{int((got != want).any(1).sum())} of {p.shape[0]} weight rows differ"


def check_gradients(dev, v, f, p, g, idx=np.int64):
    d2, I, C, gP, gV = run(dev, v, f, p, g, idx)
    want = dg.gradients(p, v, f, I.cpu().numpy(), C.cpu().numpy(), g)
    assert gP.dtype == torch.float32 and gV.dtype == torch.float32 and gP.shape == p.shape and gV.shape == v.shape
    gP, gV = gP.cpu().numpy().astype(np.float64), gV.cpu().numpy().astype(np.float64)
    assert np.isfinite(gP).all() and np.isfinite(gV).all()
    # to P: one term, no sum -- the slack alone
    err = np.abs(gP - want["gP"])
    print(f"gP: largest error / |term| {float((err / np.maximum(np.abs(want['gP']), 1e-300)).max()):.3e}")
    assert (err <= 16 * 2.0 ** -24 * np.abs(want["gP"].astype(np.float64))).all()
    # to V: the fp32 chain of the face rows and the vertex's corners
    err = np.abs(gV - want["gV"])
    bound = (want["depth"][:, None] + 16) * 2.0 ** -24 * want["abs"]
    nz = want["abs"] > 0
    print(f"gV: largest error / bound {float((err[nz] / bound[nz]).max()) if nz.any() else 0.0:.3e}, deepest chain {int(want['depth'].max())}")
    assert (err <= bound).all()
    return d2, I, C


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("name", SMALL)
def test_gradients_against_the_statement(dev, name, idx):
    """|dev - ref| <= (depth + 16) 2^-24 sum |terms| for every element; `single` puts every probe on one face (the wave path of the face
    sum), `degenerate` has repeated indices and collinear corners, the probes on vertices and edges exercise the tie rule"""
    v, f, p, _, _, g = case(name, dev)
    check_gradients(dev, v, f, p, g, idx)


def test_no_points_and_fewer_points_than_faces(dev):
    v, f, p, _, _, g = case("ico", dev)
    _, _, _, gP, gV = run(dev, v, f, p[:0], g[:0])
    assert gP.shape == (0, 3) and gV.shape == v.shape and not bool(gV.any())
    few = np.concatenate([p[3 * N:3 * N + 20], p[:5]])            # 25 points, 1280 faces: most faces get none
    check_gradients(dev, v, f, few, g[:25])
    _, I, _, _, gV = run(dev, v, f, few, g[:25])
    touched = np.zeros(v.shape[0], dtype=bool)
    touched[f[I.cpu().numpy()].reshape(-1)] = True
    assert not bool(gV[torch.from_numpy(~touched).to(dev)].any())


def test_only_one_input_requires_grad(dev):
    v, f, p, _, _, g = case("torus", dev)
    both = run(dev, v, f, p, g)
    only_p = run(dev, v, f, p, g, need_v=False)
    only_v = run(dev, v, f, p, g, need_p=False)
    assert only_p[4] is None and torch.equal(bits(only_p[3]), bits(both[3]))
    assert only_v[3] is None and torch.equal(bits(only_v[4]), bits(both[4]))


def test_two_runs_and_another_stream_give_identical_bits(dev):
    v, f, p, _, _, g = case("single", dev)
    v2, f2, p2, _, _, g2 = case("ico", dev)
    first = [run(dev, v, f, p, g), run(dev, v2, f2, p2, g2)]
    again = [run(dev, v, f, p, g), run(dev, v2, f2, p2, g2)]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        other = [run(dev, v, f, p, g), run(dev, v2, f2, p2, g2)]
    torch.cuda.current_stream(dev).wait_stream(s)
    for a, b, c in zip(first, again, other):
        for x, y, z in zip(a, b, c):
            assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))


def test_a_captured_forward_and_backward_replays_bitwise(dev):
    from largesteps.distance import MeshDistance
    v, f, p, _, _, g = case("ico", dev)
    V = torch.from_numpy(v).to(dev).requires_grad_()
    P = torch.from_numpy(p).to(dev).requires_grad_()
    G = torch.from_numpy(g).to(dev)
    with MeshDistance(V, torch.from_numpy(f).to(dev)) as m:
        def step():
            d2, I, C = m.squared_distance(P)
            gP, gV = torch.autograd.grad((d2 * G).sum(), (P, V))
            return d2.detach(), I, C, gP, gV
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
        for a, b in zip(eager, out):
            assert torch.equal(bits(a), bits(b))


def test_update_answers_like_a_fresh_handle_and_fences_the_backward(dev):
    from largesteps.distance import MeshDistance
    v, f, p, _, _, g = case("ico", dev)
    v2 = (synthetic.perturb(v, radial=0.08, seed=9).astype(F32) + F32(0.25)).astype(F32)
    tf, P = torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev)
    V1, V2 = torch.from_numpy(v).to(dev).requires_grad_(), torch.from_numpy(v2).to(dev).requires_grad_()
    with MeshDistance(V1, tf) as m, MeshDistance(V2, tf) as fresh:
        stale = m.squared_distance(P)[0]
        m.update(V2)
        for a, b in zip(m.squared_distance(P), fresh.squared_distance(P)):
            assert torch.equal(bits(a.detach()), bits(b.detach()))
        with pytest.raises(RuntimeError, match="updated"):
            stale.sum().backward()
        # the gradients after the update are those of the fresh handle, and flow into V2
        ga, = torch.autograd.grad(m.squared_distance(P)[0].sum(), V2)
        gb, = torch.autograd.grad(fresh.squared_distance(P)[0].sum(), V2)
        assert torch.equal(bits(ga), bits(gb))
        with pytest.raises(ValueError):
            m.update(V2[:-1])
        # an in-place change of the source without update
        d2 = m.squared_distance(P)[0]
        with torch.no_grad():
            V2.mul_(1.5)
        with pytest.raises(RuntimeError, match="in place"):
            d2.sum().backward()
        with pytest.raises(RuntimeError, match="in place"):
            m.squared_distance(P)
        m.update(V2)
        m.squared_distance(P)[0].sum().backward()


def test_nothing_requires_grad_is_the_plain_query(dev):
    from largesteps import _native
    from largesteps.distance import MeshDistance, point_mesh_squared_distance
    v, f, p, _, _, _ = case("folded", dev)
    V, tf, P = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev)
    n = p.shape[0]
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    I = torch.empty(n, dtype=torch.int64, device=dev)
    C = torch.empty((n, 3), dtype=torch.float64, device=dev)
    with MeshDistance(V, tf) as m:
        _native.check(_native.lib().ls_mesh_distance_query(m._h, _native.ptr(P), n, _native.ptr(d2), _native.ptr(I), _native.ptr(C), _native.stream_of(dev)))
        got = m.squared_distance(P)
        Vg = V.clone().requires_grad_()
        with torch.no_grad(), MeshDistance(Vg, tf) as mg:
            quiet = mg.squared_distance(P.clone().requires_grad_())
    for out in (got, quiet, point_mesh_squared_distance(P, V, tf)):
        assert out[0].requires_grad is False and out[0].grad_fn is None
        for a, b in zip(out, (d2, I, C)):
            assert torch.equal(bits(a), bits(b))
    # and the differentiable path returns the same bits
    for a, b in zip(point_mesh_squared_distance(P.clone().requires_grad_(), V, tf), (d2, I, C)):
        assert torch.equal(bits(a.detach()), bits(b))
    out = point_mesh_squared_distance(p, v, f)
    assert isinstance(out[0], np.ndarray) and np.array_equal(out[0], d2.cpu().numpy())


def test_the_workspace_is_checked(dev):
    from largesteps import _native
    from largesteps.distance import MeshDistance
    v, f, p, I, C, g = case("torus", dev)
    P, tI, tC, G = (torch.from_numpy(x).to(dev) for x in (p, I, C, g))
    with MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) as m:
        vptr, order = m._corner_ranks()
        gV = torch.empty((v.shape[0], 3), dtype=torch.float32, device=dev)
        need = ctypes.c_size_t(0)
        _native.check(_native.lib().ls_mesh_distance_backward_workspace_bytes(p.shape[0], f.shape[0], ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        args = (m._h, _native.ptr(P), p.shape[0], _native.ptr(tI), _native.ptr(tC), _native.ptr(G), _native.ptr(vptr), _native.ptr(order), None,
                _native.ptr(gV), _native.ptr(ws))
        assert _native.lib().ls_mesh_distance_backward(*args, need.value - 1, _native.stream_of(dev)) == _native.LS_E_WORKSPACE
        assert _native.lib().ls_mesh_distance_backward(*args, need.value, _native.stream_of(dev)) == 0
        torch.cuda.synchronize(dev)


def test_a_two_sided_fit_decreases_its_loss(dev):
    """the ico mesh against a radially perturbed copy: 20 steps of from_differential -> two-sided loss -> backward -> AdamUniform, with
    update on the moving mesh's handle at every step"""
    from largesteps.distance import MeshDistance, point_mesh_squared_distance
    from largesteps.geometry import compute_matrix
    from largesteps.optimize import AdamUniform
    from largesteps.parameterize import from_differential, to_differential
    v0, f0 = synthetic.icosphere(8)
    target = torch.from_numpy(synthetic.perturb(v0, radial=0.05, seed=2).astype(F32)).to(dev)
    v, f = torch.from_numpy(v0.astype(F32)).to(dev), torch.from_numpy(f0).to(dev)
    M = compute_matrix(v, f, lambda_=10.0)
    u = to_differential(M, v).clone().requires_grad_()
    opt = AdamUniform([u], lr=3e-3)
    losses = []
    with MeshDistance(target, f) as m_target, MeshDistance(v, f) as m_moving:
        for _ in range(21):
            x = from_differential(M, u, "Cholesky")
            m_moving.update(x)
            loss = m_target.squared_distance(x)[0].mean() + m_moving.squared_distance(target)[0].mean()
            losses.append(float(loss))
            if len(losses) == 21:
                break
            opt.zero_grad()
            loss.backward()
            opt.step()
        # the one-shot form of the second term gives the same value
        same = m_target.squared_distance(x)[0].mean() + point_mesh_squared_distance(target, x, f)[0].mean()
        assert float(same) == losses[-1]
    print(f"loss {losses[0]:.6e} -> {losses[-1]:.6e}")
    assert losses[-1] < losses[0]
