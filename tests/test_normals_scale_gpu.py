"""
csrc/normals.hip past one sweep of its reductions, against the fp64 statement (oracle/normals.py) on the jittered planes of
tests/normals_scale_cases.py -- the smallest meshes at which

    n = 364   (263,538 faces)    the looping kernels of the general path (k_edge_norm_partials, k_vertex_normals_bwd1) take a second pass,
    n = 726   (1,051,250 faces)  the pair path hands k_finish3 G = 1027 partials: its threads use their second unrolled slot,
    n = 1450  (4,199,202 faces)  G = 4101: k_finish3's loop takes a second trip.

a. the three global norms through the C ABI, relative 5e-7 (derived below), after asserting FROM THE STATEMENT that losing the partials
   in question moves the norms by >= 100 x that;
b. gN through ls_normals_pair_backward_faces with the output gradient x 1000 on the faces of the reduction's tail, against the
   statement's sum of the same per-face terms (from the device's own g_raw and the norms it was given);
c. the Python API end to end at n = 364 and 726, pair and general path, at the bounds of test_hip_large_mesh_vs_oracle_and_errors --
   and the part of the vertex gradient those bounds cannot see: with the face normals held constant only the corner angles and the
   three norms carry gradient, 7e-4 against 1.6e3 through the face normals.
Every case prints its worst |dev - ref| / tol (pytest -s).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import normals_scale_cases as nc  # noqa: E402
from oracle import normals as on  # noqa: E402

pytestmark = pytest.mark.gpu

# a. Derived, not measured. The edge subtractions are exact or within 1 ulp, each fp32 square carries <= 2^-24 and the sum is in double:
# the value before the final cast and sqrtf is within 3e-8; the cast and sqrtf add <= 1.2e-7. 5e-7 is about 3 x that. (The reference's own
# fp32 torch.norm is off by 6e-6 / 5e-5 / 4e-4 on these meshes: the kernel is held to its double accumulation, not to that.)
TOL_NORMS = 5e-7
# b. |gN_dev - gN_64| <= TOL_GN[n] * max |gN_64|. Measured (tests/golden/make_golden_normals.py --scale): the same per-face terms formed
# in numpy fp32 and summed in fp64 deviate from the fp64 statement, on these very inputs, by 7.773e-08 (n = 726) and 1.618e-07
# (n = 1450) of max |gN_64|. The tolerance is 8 x that: the margin covers rsqrtf / acosf and the order of operations.
TOL_GN = {726: 8 * 7.773e-08, 1450: 8 * 1.618e-07}
# c. the vertex gradient with the face normals constant, relative to max |gv_64|. The reference is not exact here: its fp32 result (run on
# the CPU on these meshes, make_golden_normals.py --scale) deviates from fp64 by 6.552e-05 (n = 364) and 4.761e-04 (n = 726) -- its fp32
# global norms. The tolerance is 2 x that; the kernels sum the norms in double and have no reason to be worse.
TOL_BLIND = {364: 2 * 6.552e-05, 726: 2 * 4.761e-04}
assert tuple(TOL_BLIND) == nc.END_TO_END


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def report(name, ratio):
    print(f"{name}: max |dev - ref| / tol = {ratio:.3g}")


class Case:
    """a mesh and the statement's fp64 forward on it, computed once per module and never written to"""

    def __init__(self, n):
        self.n = n
        self.v, self.f = nc.jittered_plane(n)
        self.F, self.V = self.f.shape[0], self.v.shape[0]
        self.G = nc.pair_G(self.F)
        # nc.pair_G uses PF and BLOCK as read from csrc/ (normals_scale_cases.py): a change of them fails here, not un-tests a path;
        # tests/test_normals.py::test_scale_meshes_cross_the_compiled_thresholds holds FIN, FIN_U and MESH_MAXG to these counts
        assert (self.F, self.V, self.G) == nc.SIZES[n]
        self.fn64 = on.face_normals(self.v, self.f)
        self.N64 = on.edge_norms(self.v, self.f)

    @functools.cached_property
    def forward(self):
        return on.vertex_normals(self.v, self.f, self.fn64, return_raw=True)

    @functools.cached_property
    def backward(self):
        """(gv: through the angles and the norms only, gfn, g_all) for nc.plain_weights"""
        gv, gfn = on.vertex_normals_backward(self.v, self.f, self.fn64, nc.plain_weights(self.n, self.V))
        return gv, gfn, gv + on.face_normals_backward(self.v, self.f, gfn)


@functools.lru_cache(maxsize=None)
def case(n):
    return Case(n)


def _mesh_on(c, dev):
    from largesteps import normals
    tv, tf = _t(c.v, dev), _t(c.f.astype(np.int32), dev)
    vv, ff, vptr, cpos, order = normals._prep(tv, tf)
    return vv, ff, vptr, cpos, order, normals._workspace(c.F, c.V, dev)


def _norms_check(name, norms, c, kept):
    """`kept`: the faces whose partials a reduction that loses its tail would still see (None: nothing to lose at this size)"""
    if kept is not None:
        lost = np.abs(on.edge_norms(c.v, c.f[:kept]) - c.N64) / c.N64
        assert lost.min() >= 100 * TOL_NORMS, f"{name}: the tail of the reduction moves the norms by {lost}: the comparison could not see its loss"
    err = np.abs(norms.astype(np.float64) - c.N64) / c.N64
    report(name, err.max() / TOL_NORMS)
    assert err.max() <= TOL_NORMS, (err, norms, c.N64)


@pytest.mark.parametrize("n", list(nc.SIZES))
def test_pair_norms_vs_statement(dev, n):
    from largesteps import _native
    c = case(n)
    vv, ff, _, _, _, ws = _mesh_on(c, dev)
    lib, p = _native.lib(), _native.ptr
    fn, norms = torch.zeros((3, c.F), device=dev), torch.zeros(3, device=dev)
    _native.check(lib.ls_face_normals_with_norms(p(vv), p(ff), ff.element_size(), c.F, c.V, p(fn), p(norms), p(ws), ws.numel(), dev.index,
                                                 _native.stream_of(dev)))
    torch.cuda.synchronize()
    _norms_check(f"norms pair n={n} G={c.G}", norms.cpu().numpy(), c, nc.tail_start(n))
    assert np.abs(fn.cpu().numpy() - c.fn64).max() <= 2e-6


def test_general_norms_vs_statement(dev):
    """ls_vertex_normals at n = 364: 1,394 faces are left to the second pass of k_edge_norm_partials's loop"""
    from largesteps import _native
    c = case(364)
    assert c.F - nc.GENERAL_SWEEP == 1394
    vv, ff, vptr, cpos, _, ws = _mesh_on(c, dev)
    lib, p = _native.lib(), _native.ptr
    fn = _t(c.fn64.astype(np.float32), dev)
    out, raw, norms = torch.zeros((c.V, 3), device=dev), torch.zeros((c.V, 3), device=dev), torch.zeros(3, device=dev)
    _native.check(lib.ls_vertex_normals(p(vv), p(ff), ff.element_size(), c.F, c.V, p(vptr), p(cpos), p(fn), p(out), p(raw), p(norms), p(ws),
                                        ws.numel(), dev.index, _native.stream_of(dev)))
    torch.cuda.synchronize()
    _norms_check("norms general n=364", norms.cpu().numpy(), c, nc.GENERAL_SWEEP)
    assert np.abs(out.cpu().numpy() - c.forward[0]).max() <= 5e-6


@pytest.mark.parametrize("n", [726, 1450])
def test_pair_norm_gradients_vs_statement(dev, n):
    """gN and the per-face gradient of the face normals from ls_normals_pair_backward_faces. raw, norms and g_out are inputs: built
    by tests/normals_scale_cases.py, the norms the statement's rounded to fp32; g_out is 1000 x larger on the vertices of the faces whose
    partials k_finish3 reads last."""
    from largesteps import _native
    c = case(n)
    tail = nc.tail_start(n)
    assert tail == {726: 1024, 1450: 4096}[n] * 1024 and tail < c.F
    raw32, N32 = nc.tail_raw(n, c.V), c.N64.astype(np.float32)
    w = nc.tail_weights(n, c.V, c.f)
    vv, ff, _, _, _, ws = _mesh_on(c, dev)
    lib, p = _native.lib(), _native.ptr
    g_raw, gN, gfn = torch.zeros((c.V, 3), device=dev), torch.zeros(4, device=dev), torch.zeros((3, c.F), device=dev)
    d_raw, d_norms, d_w = _t(raw32, dev), _t(N32, dev), _t(w, dev)
    _native.check(lib.ls_normals_pair_backward_faces(p(vv), p(ff), ff.element_size(), c.F, c.V, p(d_raw), p(d_norms), p(d_w), p(g_raw), p(gN),
                                                     p(gfn), p(ws), ws.numel(), dev.index, _native.stream_of(dev)))
    torch.cuda.synchronize()
    g_raw = g_raw.cpu().numpy()
    g_raw64 = on.normalize_rows_backward(raw32, w)
    assert np.abs(g_raw - g_raw64).max() <= 1e-5 * np.abs(g_raw64).max()
    # the statement on the device's own g_raw and the norms it was given: what remains are the per-face terms and the reduction
    t = on.corner_terms(c.v, c.f, c.fn64, g_raw, norms=N32)
    full, head = t["gN"].sum(axis=1), t["gN"][:, :tail].sum(axis=1)
    assert np.allclose(head, on.norm_gradients(c.v, c.f, c.fn64, g_raw=g_raw, norms=N32, faces=(tail - 2048, tail))
                       + t["gN"][:, :tail - 2048].sum(axis=1), rtol=1e-9, atol=0)
    scale = np.abs(full).max()
    tol = TOL_GN[n] * scale
    assert (np.abs(head - full) >= 10 * tol).all(), f"the tail carries {np.abs(head - full) / tol} tolerances: too little to see its loss"
    got = gN[:3].cpu().numpy().astype(np.float64)
    report(f"gN pair n={n} G={c.G}", np.abs(got - full).max() / tol)
    # per face, in the form of test_hip_vs_reference (1e-5 max |.|) -- the faces that touch a vertex with the 1000 x larger g_out (the
    # tail's and the row next to it) and all others against their OWN maximum: the former's would leave the latter unchecked
    gfn = gfn.cpu().numpy()
    scaled = np.zeros(c.V, dtype=bool)
    scaled[nc.tail_vertices(n, c.f)] = True
    big = scaled[c.f].any(axis=1)
    assert np.abs(t["grad_fn"][:, big]).max() > 100 * np.abs(t["grad_fn"][:, ~big]).max() and (~big).sum() > 0.99 * tail
    e_fn = max(np.abs(gfn[:, r] - t["grad_fn"][:, r]).max() / (1e-5 * np.abs(t["grad_fn"][:, r]).max()) for r in (big, ~big))
    report(f"grad_fn per face n={n}", e_fn)
    assert np.abs(got - full).max() <= tol, (got, full, head)
    assert e_fn <= 1.0

@pytest.mark.parametrize("pair", [True, False], ids=["pair", "general"])
@pytest.mark.parametrize("n", nc.END_TO_END)
def test_api_end_to_end_vs_statement(dev, n, pair, monkeypatch):
    from largesteps.normals import compute_face_normals, compute_vertex_normals
    if not pair:
        monkeypatch.setenv("LARGESTEPS_NORMALS_PAIR", "0")
    c = case(n)
    name = f"n={n} {'pair' if pair else 'general'}"
    vn64 = c.forward[0]
    gv64, gfn64, g64 = c.backward
    w = _t(nc.plain_weights(n, c.V), dev)
    tv, tf = _t(c.v, dev).requires_grad_(True), _t(c.f, dev)

    def run():
        fn = compute_face_normals(tv, tf)
        vn = compute_vertex_normals(tv, tf, fn)
        g, = torch.autograd.grad((vn * w).sum(), tv)
        return fn.detach(), vn.detach(), g

    fn, vn, g = run()
    e = (np.abs(fn.cpu().numpy() - c.fn64).max() / 2e-6, np.abs(vn.cpu().numpy() - vn64).max() / 5e-6,
         np.abs(g.cpu().numpy() - g64).max() / (2e-4 * np.abs(g64).max()))
    report(f"fn {name}", e[0]), report(f"vn {name}", e[1]), report(f"g_all {name}", e[2])
    assert max(e) <= 1.0, e
    for a, b in zip(run(), (fn, vn, g)):                      # no atomics anywhere: the same bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the blind spot of the bound on g_all: the face normals as a constant, then as an independent leaf -- only the corner angles and
    # the three global norms carry gradient to the vertices (max |gv| ~ 5e-4 next to max |g_all| ~ 2e3)
    assert np.abs(gv64).max() < 1e-5 * np.abs(g64).max()
    tol = TOL_BLIND[n] * np.abs(gv64).max()
    with torch.no_grad():
        fn_c = compute_face_normals(tv, tf)
    g_const, = torch.autograd.grad((compute_vertex_normals(tv, tf, fn_c) * w).sum(), tv)
    fn_c.requires_grad_(True)
    g_leaf, g_leaf_fn = torch.autograd.grad((compute_vertex_normals(tv, tf, fn_c) * w).sum(), (tv, fn_c))
    e_const, e_leaf = np.abs(g_const.cpu().numpy() - gv64).max() / tol, np.abs(g_leaf.cpu().numpy() - gv64).max() / tol
    report(f"gv, fn constant {name}", e_const), report(f"gv, fn a leaf {name}", e_leaf)
    assert e_const <= 1.0 and e_leaf <= 1.0
    assert np.abs(g_leaf_fn.cpu().numpy() - gfn64).max() <= 1e-5 * np.abs(gfn64).max()
