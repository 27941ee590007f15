"""
Same-pattern refactorisation of the nested-dissection direct solver on the MI355X: ls_direct_factor_refactorable / ls_direct_refactor
through the C ABI, NestedDissectionSolver.refactor / CholeskySolver.refactor, and parameterize.update_matrix. A refactor of matrix B on a
handle built from matrix A must be bitwise a fresh factorisation of B (same positions, same options), accurate against the fp64 oracle,
refuse a different pattern, survive a matrix that is not positive definite, keep every device address (graph replay), guard autograd
and leave no device memory behind.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import solve as osv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kw(c, **over):
    kw = dict(lambda_=c["lambda_"] if c["lambda_"] is not None else 0.0, alpha=c["alpha"], cotan=c["cotan"])
    kw.update(over)
    return kw


def _pair(name, dev):
    """(positions, A, B) of a config: B has A's pattern and other values -- the cotangent config re-linearised on perturbed vertices,
    the others with another lambda."""
    from largesteps import synthetic
    from largesteps.geometry import compute_matrix
    v, f, c = synthetic.config_mesh(name)
    tv, tf = _t(v, dev), _t(f, dev)
    A = compute_matrix(tv, tf, **_kw(c))
    if c["cotan"]:
        v2 = synthetic.perturb(v, radial=0.01, seed=7).astype(np.float32)
        B = compute_matrix(_t(v2, dev), tf, **_kw(c))
    else:
        B = compute_matrix(tv, tf, **_kw(c, lambda_=1.9 * c["lambda_"] + 1.0))
    assert torch.equal(A.indices(), B.indices()) and not torch.equal(A.values(), B.values())
    return tv, A, B


class _Abi:
    """Raw C-ABI caller: explicit options (ordering = LS_ND_ORDER_LONGEST), handles destroyed at the end."""

    def __init__(self, dev):
        from largesteps import _native
        self.n, self.lib, self.dev, self.handles = _native, _native.lib(), dev, []

    def factor(self, csr, pos, refactorable):
        n = self.n
        opt = n.DirectOptions()
        n.check(self.lib.ls_direct_options_default(ctypes.byref(opt)))
        opt.ordering = 0
        h = ctypes.c_void_p()
        fn = self.lib.ls_direct_factor_refactorable if refactorable else self.lib.ls_direct_factor_ex
        n.check(fn(n.ptr(csr.rowptr), n.ptr(csr.col), n.ptr(csr.val), csr.V, csr.nnz, n.ptr(pos), ctypes.byref(opt), self.dev.index,
                   n.stream_of(self.dev), ctypes.byref(h)))
        self.handles.append(h)
        return h

    def solve_rc(self, h, b):
        x = torch.empty_like(b)
        rc = self.lib.ls_direct_solve(h, b.data_ptr(), x.data_ptr(), b.shape[1], self.n.raw_stream(self.dev))
        torch.cuda.synchronize(self.dev)
        return rc, x

    def solve(self, h, b):
        rc, x = self.solve_rc(h, b)
        self.n.check(rc)
        return x

    def refactor(self, h, csr):
        n = self.n
        return self.lib.ls_direct_refactor(h, n.ptr(csr.rowptr), n.ptr(csr.col), n.ptr(csr.val), csr.V, csr.nnz, n.stream_of(self.dev))

    def refactorable(self, h):
        yes, kept = ctypes.c_int(-1), ctypes.c_size_t(0)
        self.n.check(self.lib.ls_direct_refactorable(h, ctypes.byref(yes), ctypes.byref(kept)))
        return yes.value, kept.value

    def launches(self, h):
        nl = ctypes.c_int(0)
        self.n.check(self.lib.ls_direct_info(h, None, ctypes.byref(nl), None))
        return nl.value

    def close(self):
        for h in self.handles:
            self.lib.ls_direct_destroy(h)
        self.handles = []


@pytest.fixture
def abi(dev):
    a = _Abi(dev)
    yield a
    a.close()


def _rhs(V, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((V, 3), generator=g, dtype=torch.float32).to(dev)


@pytest.mark.parametrize("name", ["cfg1_icosphere2k", "cfg2_bunny70k", "cfg3_dragon250k", "cfg4_plane1m"])
def test_refactor_is_bitwise_a_fresh_factorisation_and_accurate(dev, abi, name):
    """A refactorable handle of A, refactored to B, solves bit for bit like ls_direct_factor_ex(B) with the same positions and options
    (one dense node; dense arity-8 leaves; the cotangent matrix on moved vertices; the 16-wave tier with sparse leaves), and within
    1e-4 of the fp64 oracle's solution of B."""
    from largesteps import _native
    tv, A, B = _pair(name, dev)
    ca, cb = _native.csr_of(A), _native.csr_of(B)
    assert torch.equal(ca.rowptr, cb.rowptr) and torch.equal(ca.col, cb.col)
    h = abi.factor(ca, tv, True)
    yes, kept = abi.refactorable(h)
    assert yes == 1 and kept > 0
    b = _rhs(ca.V, dev)
    xa = abi.solve(h, b)
    assert abi.refactor(h, cb) == 0, _native.last_error()
    x = abi.solve(h, b)
    fresh = abi.factor(cb, tv, False)
    assert torch.equal(x, abi.solve(fresh, b)), name
    assert not torch.equal(x, xa)
    assert abi.refactor(h, ca) == 0                          # and back: bitwise the handle it was
    assert torch.equal(abi.solve(h, b), xa)
    idx, val = B.indices().cpu().numpy(), B.values().cpu().numpy()
    x64 = osv.DirectSolver(idx[0], idx[1], val, ca.V).solve(b.cpu().numpy())
    err = np.abs(x.cpu().numpy() - x64).max()
    assert err <= 1e-4 * np.abs(x64).max(), (name, err)


@pytest.mark.parametrize("name", ["cfg2_bunny70k", "cfg4_plane1m"])
def test_retention_changes_nothing(dev, abi, name):
    """What a refactorable handle keeps does not change its factor or its solve: torch.equal solves, the same launch count."""
    from largesteps import _native
    tv, A, _ = _pair(name, dev)
    csr = _native.csr_of(A)
    hr, hp = abi.factor(csr, tv, True), abi.factor(csr, tv, False)
    assert abi.refactorable(hp) == (0, 0)
    b = _rhs(csr.V, dev, 1)
    assert torch.equal(abi.solve(hr, b), abi.solve(hp, b))
    assert abi.launches(hr) == abi.launches(hp)


def _edit_pattern(M, mode):
    """M with one off-diagonal pair (i, j), (j, i) added, removed or moved (removed + another added: the same nnz). The matrix stays
    symmetric and diagonally dominant."""
    idx, val = M.indices().cpu(), M.values().cpu()
    V = M.shape[0]
    r, c = idx[0], idx[1]
    keep = torch.ones(val.shape[0], dtype=torch.bool)
    if mode in ("removed", "moved"):
        e = int(torch.nonzero(r < c)[0])
        i, j = int(r[e]), int(c[e])
        keep &= ~(((r == i) & (c == j)) | ((r == j) & (c == i)))
    idx, val = idx[:, keep], val[keep]
    if mode in ("added", "moved"):
        have = set(zip(r.tolist(), c.tolist()))
        i = 0
        j = next(j for j in range(V - 1, 0, -1) if (i, j) not in have)
        idx = torch.cat([idx, torch.tensor([[i, j], [j, i]])], 1)
        val = torch.cat([val, torch.tensor([-1e-3, -1e-3])])
    return torch.sparse_coo_tensor(idx, val, (V, V)).coalesce().to(M.device)


@pytest.mark.parametrize("mode", ["added", "removed", "moved"])
def test_pattern_mismatch_is_refused_and_the_factor_kept(dev, abi, mode):
    from largesteps import _native
    from largesteps.solvers import NestedDissectionSolver
    tv, A, _ = _pair("cfg2_bunny70k", dev)
    C = _edit_pattern(A, mode)
    ca, cc = _native.csr_of(A), _native.csr_of(C)
    h = abi.factor(ca, tv, True)
    b = _rhs(ca.V, dev, 2)
    x0 = abi.solve(h, b)
    assert abi.refactor(h, cc) == _native.LS_E_INVALID
    assert "pattern differs" in _native.last_error()
    assert torch.equal(abi.solve(h, b), x0)
    s = NestedDissectionSolver(A, refactorable=True, ordering="longest-axis")
    y0 = s.solve(b)
    with pytest.raises(ValueError, match="pattern"):
        s.refactor(C)
    assert s.factored and s.generation == 0
    assert torch.equal(s.solve(b), y0)


def test_not_positive_definite_leaves_the_handle_unfactored_until_a_refactor_succeeds(dev, abi):
    from largesteps import _native
    from largesteps.geometry import compute_matrix
    from largesteps.solvers import NestedDissectionSolver
    from largesteps import synthetic
    tv, A, B = _pair("cfg2_bunny70k", dev)
    _, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    A10 = compute_matrix(tv, _t(f, dev), 10.0)                    # I + 10 L
    idx = A10.indices()
    diag = (idx[0] == idx[1]).to(torch.float32)
    C = torch.sparse_coo_tensor(idx, 2.0 * diag - A10.values(), A10.shape).coalesce()      # I - 10 L
    ca, cb, cc = _native.csr_of(A), _native.csr_of(B), _native.csr_of(C)
    b = _rhs(ca.V, dev, 3)
    h = abi.factor(ca, tv, True)
    assert abi.refactor(h, cc) == _native.LS_E_INVALID
    assert "positive definite" in _native.last_error()
    assert abi.solve_rc(h, b)[0] == _native.LS_E_STATE
    assert abi.refactor(h, cb) == 0
    assert torch.equal(abi.solve(h, b), abi.solve(abi.factor(cb, tv, False), b))
    s = NestedDissectionSolver(A, refactorable=True, ordering="longest-axis")
    with pytest.raises(ValueError, match="positive definite"):
        s.refactor(C)
    assert not s.factored
    with pytest.raises(RuntimeError, match="unfactored"):
        s.solve(b)
    s.refactor(B)
    assert s.factored and s.generation == 1
    assert torch.equal(s.solve(b), NestedDissectionSolver(B, ordering="longest-axis").solve(b))


def test_handles_that_cannot_refactor(dev, abi):
    from largesteps import _native
    from largesteps.solvers import CholeskySolver, NestedDissectionSolver
    tv, A, B = _pair("cfg1_icosphere2k", dev)
    ca, cb = _native.csr_of(A), _native.csr_of(B)
    h = abi.factor(ca, tv, False)
    assert abi.refactorable(h) == (0, 0)
    assert abi.refactor(h, cb) == _native.LS_E_STATE
    assert "ls_direct_factor_refactorable" in _native.last_error()
    with pytest.raises(RuntimeError, match="refactorable=False"):
        NestedDissectionSolver(A).refactor(B)
    with pytest.raises(RuntimeError, match="refactorable=False"):
        CholeskySolver(A).refactor(B)


def test_iterative_fallback_is_rebuilt_by_refactor(dev):
    from largesteps.solvers import CholeskySolver, IterativeCholeskySolver
    tv, A, B = _pair("cfg1_icosphere2k", dev)
    s = CholeskySolver(A, direct=False, refactorable=True)
    assert isinstance(s._impl, IterativeCholeskySolver)
    s.refactor(B)
    assert s.generation == 1 and isinstance(s._impl, IterativeCholeskySolver)
    b = _rhs(tv.shape[0], dev, 4)
    idx, val = B.indices().cpu().numpy(), B.values().cpu().numpy()
    x64 = osv.DirectSolver(idx[0], idx[1], val, tv.shape[0]).solve(b.cpu().numpy())
    assert np.abs(s.solve(b).cpu().numpy() - x64).max() <= 1e-4 * np.abs(x64).max()


def test_captured_graph_replays_with_the_updated_matrix(dev):
    """from_differential (forward and backward) captured into a graph, then update_matrix(M, M2): the replay solves M2, bit for bit
    what an eager from_differential(M2, u) on the same solver gives."""
    from largesteps import parameterize
    from largesteps.parameterize import from_differential, to_differential, update_matrix
    tv, M, M2 = _pair("cfg2_bunny70k", dev)
    update_matrix(M, M)                                            # the solver cached for M: a refactorable one
    solver = parameterize._cache[(id(M), "Cholesky")][0]
    assert solver.refactorable
    u = to_differential(M, tv).detach().clone().requires_grad_(True)
    w = _rhs(tv.shape[0], dev, 5)

    def step():
        x = from_differential(M, u)
        (x * w).sum().backward()
        return x

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            u.grad = None
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    u.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x_static = step()
    update_matrix(M, M2)
    assert parameterize._cache[(id(M2), "Cholesky")][0] is solver and (id(M), "Cholesky") not in parameterize._cache
    u.grad.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    u2 = u.detach().clone().requires_grad_(True)
    x2 = from_differential(M2, u2)
    (x2 * w).sum().backward()
    assert torch.equal(x_static, x2)
    assert torch.equal(u.grad, u2.grad)


def test_update_matrix_autograd(dev):
    """After update_matrix the cached solver is the same object (no construction: its timings are unchanged), gradients through
    from_differential(M2, u) match the fp64 oracle, and a backward through a graph built before the update raises."""
    from largesteps import parameterize
    from largesteps.parameterize import from_differential, to_differential, update_matrix
    tv, M, M2 = _pair("cfg2_bunny70k", dev)
    assert update_matrix(M, M) is M
    solver = parameterize._cache[(id(M), "Cholesky")][0]
    timings, built = dict(solver.timings), solver.build_seconds
    u = to_differential(M, tv).detach().clone().requires_grad_(True)
    x_old = from_differential(M, u)
    assert update_matrix(M, M2) is M2
    assert parameterize._cache[(id(M2), "Cholesky")][0] is solver
    assert solver.timings == timings and solver.build_seconds == built
    with pytest.raises(RuntimeError, match="refactored"):
        x_old.sum().backward()
    u2 = u.detach().clone().requires_grad_(True)
    x2 = from_differential(M2, u2)
    w = _rhs(tv.shape[0], dev, 6)
    (x2 * w).sum().backward()
    idx, val = M2.indices().cpu().numpy(), M2.values().cpu().numpy()
    direct = osv.DirectSolver(idx[0], idx[1], val, tv.shape[0])
    x_ref, g_ref = direct.solve(u2.detach().cpu().numpy()), direct.solve(w.cpu().numpy())
    assert np.abs(x2.detach().cpu().numpy() - x_ref).max() <= 1e-4 * np.abs(x_ref).max()
    assert np.abs(u2.grad.cpu().numpy() - g_ref).max() <= 1e-4 * np.abs(g_ref).max()
    # no refactorable solver cached for the old matrix: one is constructed for the new one and cached
    M3 = (M2 * 1.0).coalesce()
    M4 = (M3 * 2.0).coalesce()
    update_matrix(M3, M4)
    assert parameterize._cache[(id(M4), "Cholesky")][0].refactorable
    # 'CG': the old entry is dropped
    from_differential(M4, u2.detach(), "CG")
    update_matrix(M4, M3, "CG")
    assert (id(M4), "CG") not in parameterize._cache


def test_refactors_leak_no_device_memory(dev):
    """20 alternating refactors at 250k vertices: with the pool emptied (ls_release_scratch) the device's free memory is what it was."""
    from largesteps.solvers import NestedDissectionSolver, release_scratch
    tv, A, B = _pair("cfg3_dragon250k", dev)
    s = NestedDissectionSolver(A, refactorable=True)
    s.refactor(B)

    def free():
        torch.cuda.synchronize(dev)
        release_scratch(dev)
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info(dev)[0]

    f0 = free()
    for i in range(20):
        s.refactor(A if i % 2 == 0 else B)
    f1 = free()
    assert abs(f1 - f0) <= (8 << 20), (f0, f1)
