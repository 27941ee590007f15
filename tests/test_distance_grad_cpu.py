"""
The gradient of the point-to-mesh distance without a device: tests/distance_grad_statement.py (the weights and gradients the device
must match) against its own invariants, closed forms on one triangle and torch autograd through the closest-point computation; then
the argument checks of the new C ABI entries that answer before any device work.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distance_grad_statement as dg
import distance_statement as ds
from test_distance_gpu import SMALL, mesh, probes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
N = 64                  # probes(v, f, N, seed): on_v [0, N), on_e [N, 3 N), then near, far, very far and the mirrored vertices

_cases = {}


def case(name):
    """(v, f, p, sqrD, I, C) of a SMALL mesh and its probes by the brute force, computed once"""
    if name not in _cases:
        v, f = mesh(name)
        f = np.asarray(f, dtype=np.int64)
        p = probes(v, f, N, seed=len(name))
        _cases[name] = (v, f, p) + ds.squared_distance(p, v, f)
    return _cases[name]


@pytest.mark.parametrize("name", SMALL)
def test_weights_are_a_partition_of_unity_and_reproduce_the_closest_point(name):
    """sum w = 1 within 2 ulp, w >= -2^-50, and sum_k w_k V_k = C within 32 x 2^-53 x M, M the mesh's largest coordinate. The count
    (first order, in units of 2^-53 M, every weight at most 1 and every coordinate at most M): C = (a + ab v) + ac w has the roundings of
    ab and ac (2 M each: 4), of the two products (4) and of the two sums (2): 10; the recombination has the two roundings of (1 - v) - w
    times |a| (2), three products (3) and two sums (2): 7. 17 in all, taken to the next power of two for the second-order terms: 32."""
    v, f, p, _, I, C = case(name)
    w = dg.weights(p, v, f, I)
    assert np.isfinite(w).all()
    assert (np.abs((w[:, 0] + w[:, 1]) + w[:, 2] - 1.0) <= 2 * 2.0 ** -52).all()
    assert (w >= -2.0 ** -50).all()
    v64 = v.astype(np.float64)
    back = (w[:, 0, None] * v64[f[I, 0]] + w[:, 1, None] * v64[f[I, 1]]) + w[:, 2, None] * v64[f[I, 2]]
    M = float(np.abs(v64).max())
    assert np.abs(back - C).max() <= 32 * 2.0 ** -53 * M


def test_hand_cases_on_one_triangle():
    """a = 0, b = e_x, c = e_y: a point above the interior, beyond each edge and beyond each vertex; every number is a binary fraction,
    so the closed forms are exact"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F32)
    f = np.array([[0, 1, 2]])
    p = np.array([[0.25, 0.25, 2.0], [0.5, -1.0, 0.5], [-1.0, 0.5, 0.5], [1.0, 1.0, 0.5], [-1.0, -1.0, 1.0], [2.0, -0.5, 1.0], [-0.5, 2.0, 1.0]],
                 dtype=F32)
    want_w = np.array([[0.5, 0.25, 0.25], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    want_C = want_w @ v.astype(np.float64)
    d2, I, C = ds.squared_distance(p, v, f)
    assert np.array_equal(C, want_C)
    assert np.array_equal(dg.weights(p, v, f, I), want_w)
    g = np.array([1.0, 0.5, 2.0, 0.75, 1.5, 0.25, 3.0])
    d = p.astype(np.float64) - want_C
    for i in range(p.shape[0]):
        sel = slice(i, i + 1)
        out = dg.gradients(p[sel], v, f, I[sel], C[sel], g[sel])
        assert np.array_equal(out["gP"], (2 * g[i] * d[sel]).astype(F32))
        assert np.array_equal(out["gV"], -2 * g[i] * want_w[i][:, None] * d[i][None, :])
    # all seven at once: the vertex gradient is the sum of the seven terms
    out = dg.gradients(p, v, f, I, C, g)
    assert np.array_equal(out["gV"], np.einsum("i,ik,iq->kq", -2 * g, want_w, d))
    assert np.array_equal(out["depth"], [7 + 1] * 3)


def test_a_repeated_index_receives_both_of_its_weights():
    v = np.array([[0, 0, 0], [2, 0, 0]], dtype=F32)
    f = np.array([[0, 0, 1]])
    p = np.array([[0.5, 1.0, 0.0]], dtype=F32)
    _, I, C = ds.squared_distance(p, v, f)[0:3]
    w = dg.weights(p, v, f, I)
    # ab is the point a (t = 0: weight 1 on the first end), bc is the segment and strictly closer: (0, 1 - 1/4, 1/4)
    assert np.array_equal(w, [[0.0, 0.75, 0.25]])
    out = dg.gradients(p, v, f, I, C, np.ones(1))
    assert np.array_equal(out["gV"], [[0, -1.5, 0], [0, -0.5, 0]])


AUTOGRAD_MEASURED = 4.742e-14          # the largest relative deviation measured on the CPU (the torus; see the docstring below)
C_ROUNDING = 32 * 2.0 ** -53            # the rounding of C in units of the mesh's largest coordinate (the count of the first test)


@pytest.mark.parametrize("name", [n for n in SMALL if n != "degenerate"])
def test_the_envelope_formula_against_autograd_through_the_closest_point(name):
    """torch autograd through distance_statement.point_face_torch differentiates |p - C(p, V)|^2 with C's dependence on p and V: the
    statement's gradient leaves that dependence out (C minimises over the face), so the two agree up to rounding. Compared per point
    (to p) and per vertex (to V) relative to the sum of the magnitudes of the row's terms, sum |2 g d|_1 over the points of the faces
    around the vertex -- the weights taken as 1, because autograd reaches a corner of weight 0 through quantities that cancel only in
    exact arithmetic (on edge bc, d4 - d3 = bc . bp does not depend on a; d4 and d3 do).
    The probes are every group that `probes` makes after on_v and on_e: near, far, very far and the mirrored vertices -v[:N]. Of these,
    a probe is left out only if it lies on the mesh to within the rounding of C itself, max |p - C| <= 32 x 2^-53 x M (M the mesh's
    largest coordinate; the bound on C's rounding that the first test derives): there p - C is rounding noise, the probe is one of
    the on-vertex probes in all but name, the gradient is not unique and a relative deviation means nothing (measured with them: 1.0).
    That happens only to mirrored vertices of meshes that a point reflection maps onto themselves: -v[k] is a vertex again, bitwise
    (|p - C| = 0) or up to a coordinate that is 1e-16 on one side and 0 on the other (|p - C| <= 6e-18). Left out: ico 0, plane 1,
    torus all 64, folded 1, tube 12, single 0; every other probe is at least 3e-4 M from the mesh, so the rule has no borderline case.
    Measured on the CPU, the largest relative deviation: ico 2.44e-14, plane 3.58e-14, torus 4.74e-14, folded 4.9e-16, tube 6.0e-16,
    single 4.5e-15, so 4.742e-14. Asserted: 16 x that."""
    v, f, p, _, I, C = case(name)
    keep = np.arange(p.shape[0]) >= 3 * N
    keep &= np.abs(p.astype(np.float64) - C).max(-1) > C_ROUNDING * float(np.abs(v).max())
    print(f"{name}: {int(keep.sum())} of {p.shape[0] - 3 * N} probes after on_v and on_e compared")
    p, I, C = p[keep], I[keep], C[keep]
    g = np.random.default_rng(5).uniform(0.5, 1.5, p.shape[0])
    tP, tV = dg.terms(p, v, f, I, C, g)
    gV, sV = np.zeros((v.shape[0], 3)), np.zeros(v.shape[0])
    for k in range(3):
        np.add.at(gV, f[I, k], tV[:, k])
        np.add.at(sV, f[I, k], np.abs(tP).sum(-1))
    sP = np.abs(tP).sum(-1)
    P = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    V = torch.from_numpy(v.astype(np.float64)).requires_grad_()
    tf, tI = torch.from_numpy(f), torch.from_numpy(I)
    q = ds.point_face_torch(P, V[tf[tI, 0]], V[tf[tI, 1]], V[tf[tI, 2]])
    assert np.array_equal(q.detach().numpy(), C)
    (torch.from_numpy(g) * ds.sq(P, q)).sum().backward()
    dev_P = np.abs(P.grad.numpy() - tP).max(-1)
    dev_V = np.abs(V.grad.numpy() - gV).max(-1)
    assert (sP > 0).all() and (dev_V[sV == 0] == 0).all()
    rel = max(float((dev_P / sP).max()), float((dev_V[sV > 0] / sV[sV > 0]).max()))
    print(f"{name}: largest relative deviation {rel:.3e}")
    assert rel <= 16 * AUTOGRAD_MEASURED


# ---- the native boundary that answers before any device work ------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


NAMES = ["ls_mesh_distance_weights", "ls_mesh_distance_backward_workspace_bytes", "ls_mesh_distance_backward", "ls_mesh_distance_update"]


def test_header_and_binding_entries(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(native.lib(), name).restype is ctypes.c_int


def test_abi_argument_checks(native):
    lib = native.lib()
    E = native.LS_E_INVALID
    buf = (ctypes.c_double * 16)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.c_void_p(1)                  # never dereferenced: every call below fails an argument check first
    assert lib.ls_mesh_distance_weights(None, x, 1, x, x, None) == E
    assert lib.ls_mesh_distance_weights(h, None, 1, x, x, None) == E
    assert lib.ls_mesh_distance_weights(h, x, 1, None, x, None) == E
    assert lib.ls_mesh_distance_weights(h, x, 1, x, None, None) == E
    assert lib.ls_mesh_distance_weights(h, x, -1, x, x, None) == E
    assert lib.ls_mesh_distance_weights(h, x, 2 ** 31, x, x, None) == native.LS_E_OVERFLOW
    assert lib.ls_mesh_distance_weights(h, None, 0, None, None, None) == 0
    n = ctypes.c_size_t(0)
    assert lib.ls_mesh_distance_backward_workspace_bytes(10, 4, None) == E
    assert lib.ls_mesh_distance_backward_workspace_bytes(-1, 4, ctypes.byref(n)) == E
    assert lib.ls_mesh_distance_backward_workspace_bytes(10, 0, ctypes.byref(n)) == E
    assert lib.ls_mesh_distance_backward_workspace_bytes(2 ** 31, 4, ctypes.byref(n)) == native.LS_E_OVERFLOW
    assert lib.ls_mesh_distance_backward_workspace_bytes(0, 4, ctypes.byref(n)) == 0 and n.value > 0
    small = n.value
    assert lib.ls_mesh_distance_backward_workspace_bytes(100000, 4000, ctypes.byref(n)) == 0
    assert n.value >= small + 100000 * (4 + 4 + 24) + 4000 * 36
    assert lib.ls_mesh_distance_backward(None, x, 1, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, None, 1, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, 1, x, None, x, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, 1, x, x, None, x, x, x, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, -1, x, x, x, x, x, x, x, x, 1 << 20, None) == E
    # the vertex gradient needs I, the corner ranking and a workspace
    assert lib.ls_mesh_distance_backward(h, x, 1, None, x, x, x, x, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, 1, x, x, x, None, x, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, 1, x, x, x, x, None, None, x, x, 1 << 20, None) == E
    assert lib.ls_mesh_distance_backward(h, x, 1, x, x, x, x, x, None, x, None, 0, None) == E and "workspace" in native.last_error()
    assert lib.ls_mesh_distance_backward(h, x, 2 ** 31, x, x, x, x, x, x, x, x, 1 << 20, None) == native.LS_E_OVERFLOW
    assert lib.ls_mesh_distance_update(None, x, None) == E
    assert lib.ls_mesh_distance_update(h, None, None) == E
