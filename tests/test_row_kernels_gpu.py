"""
The sparse row kernels on IRREGULAR rows (-m gpu). Every mesh of the other test files has valence 6 at most, so they only ever run the
short-row form of each row product; here the rows come from tests/irregular_meshes.py and reach every branch:

    row_csr_lds (csrc/spmv_kernels.h)   tiles of exactly LDS_CAP - 1, LDS_CAP and LDS_CAP + 1 entries, entry counts 1..3 modulo 4 (the scalar
                                        tail of the 16-byte copy), rows longer than the 8 gathers of one trip, an over-capacity tile
                                        before and after a staged one in the same workgroup
    k_spmv_strided (csrc/spmv.hip)      k = 5, 7, 8, 9: column groups of 4 and remainders of 1 and 3
    row_sell (PCG, k_cheb, k_resnorm)   slices wider than 8: the 4-way loop and its tail
    k_cheb_uniform                      slices wider than 8 (the plain loop)
    k_patch_cheb                        patches of width <= 6, 7, 8 and > 8 in one plan

SpMV results are held to the running error bound of their own fma chain against fp64; solver results to the project's stated
||x - x*||_inf <= 1e-4 ||x*||_inf against the fp64 direct solve. Every solve runs with warnings turned into errors: a Chebyshev
solve whose residual check fails warns and falls back to PCG, and a wrong Chebyshev kernel must not pass that way.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import irregular_meshes as im
from oracle import solve as osv

pytestmark = pytest.mark.gpu

LDS_CAP = 2560          # csrc/spmv_kernels.h
U32 = 2.0 ** -24        # unit roundoff of fp32
TOL = 1e-4              # forward error of every solve path against the fp64 direct solve


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()          # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# =====================================================================================================================================
# SpMV
# =====================================================================================================================================
def _tile(special, total, rng):
    """256 row lengths that hold `special` and add up to exactly `total`, in a seeded random order"""
    special = list(special)
    n = 256 - len(special)
    rest = total - sum(special)
    assert n > 0 and rest >= 0
    fill = np.full(n, rest // n, dtype=np.int64)
    fill[:rest % n] += 1
    out = np.concatenate([np.asarray(special, dtype=np.int64), fill])
    return out[rng.permutation(256)]


def _tiled_lengths():
    """Twelve 256-row tiles (the last one ragged: V = 3001). ls_spmv runs 12 tiles on 8 workgroups, workgroup w taking tiles 2w and
    2w + 1 one after the other through the same LDS buffer (TileSched in csrc/common.h), so the pairs below are what one workgroup sees:
        (0, 1)  exactly LDS_CAP - 1 entries (staged), then LDS_CAP + 1 (direct reads)
        (2, 3)  a row of 3000 entries (direct reads), then exactly LDS_CAP (staged: the buffer holds nothing of tile 2)
        (4, 5)  every special row length, total = 1 modulo 4; total = 2 modulo 4
        (6, 7)  total = 3 modulo 4; over capacity
        (8, 9)  staged between the over-capacity tiles 7 and 10 in memory; short rows only (what the regular meshes give)
        (10, 11) over capacity; the ragged tail (185 rows)"""
    rng = np.random.default_rng(11)
    special = [0, 1, 7, 8, 9, 12, 13, 16, 17, 64, 300]
    tiles = [_tile([], LDS_CAP - 1, rng), _tile([], LDS_CAP + 1, rng),
             _tile([3000, 0, 1], 3000 + 1 + 700, rng), _tile([17, 0], LDS_CAP, rng),
             _tile(special, 2301, rng), _tile([9, 16, 0], 1802, rng),
             _tile([13, 8], 2003, rng), _tile([64, 300, 0], 2900, rng),
             _tile([12, 1], 2048, rng), _tile([], 1500, rng),
             _tile([300, 300, 17], 2700, rng), _tile([], 1792, rng)[:185]]
    return np.concatenate(tiles)


_SPMV = {}


def _spmv_case(name, dev):
    """(M on the device, A fp64 scipy, row lengths); built once per module"""
    if name not in _SPMV:
        if name == "tiles":
            lengths = _tiled_lengths()
        else:                                            # "V<n>": short and long rows mixed, a slice or tile boundary at V - 1, V, V + 1
            V = int(name[1:])
            lengths = np.minimum(np.random.default_rng(V).integers(0, 21, size=V), V)
            if V >= 300:
                lengths[V // 2] = 300
        M, A = im.csr_with_row_lengths(lengths, seed=len(lengths), device=dev)
        _SPMV[name] = (M, A, lengths)
    return _SPMV[name]


def _raw_spmv(csr, x, variant):
    """ls_spmv into an output that is NaN everywhere before the call: an element the kernel does not write shows"""
    from largesteps import _native
    y = torch.full_like(x, float("nan"))
    _native.check(_native.lib().ls_spmv(_native.ptr(csr.rowptr), _native.ptr(csr.col), _native.ptr(csr.val), csr.V, csr.nnz, _native.ptr(x),
                                        _native.ptr(y), x.shape[1], variant, csr.device.index, _native.stream_of(csr.device)))
    return y


def _assert_within_fma_bound(y, A, x, lengths, what):
    """|y_i - (A x)_i| <= (len_i + 1) 2^-24 sum_j |a_ij x_j|: one rounding per entry of the row's fma chain (Higham, Accuracy and Stability
    of Numerical Algorithms, section 3.1: gamma_n = n u / (1 - n u) <= (n + 1) u for n <= 3000). Returns the largest error / bound."""
    x64 = x.astype(np.float64)
    y64 = A @ x64
    bound = (lengths[:, None] + 1) * U32 * (abs(A) @ np.abs(x64))
    err = np.abs(y.astype(np.float64) - y64)
    assert np.isfinite(y).all(), f"{what}: an element was not written"
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside the fma bound, first at row {int(np.argwhere(bad)[0][0])} "
                           f"(length {int(lengths[np.argwhere(bad)[0][0]])}): error {err[bad].max():.3e}")
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"[row kernels] {what}: max error / bound = {ratio:.3f}")
    return ratio


def test_the_tiled_matrix_reaches_every_branch_of_row_csr_lds():
    lengths = _tiled_lengths()
    assert lengths.shape[0] == 3001
    for n in (0, 1, 7, 8, 9, 12, 13, 16, 17, 64, 300, 3000):
        assert (lengths == n).any(), f"no row of length {n}"
    t = im.tile_entries(lengths)
    assert t.shape[0] == 12, "12 tiles on 8 workgroups: two tiles per workgroup share the LDS buffer"
    assert {LDS_CAP - 1, LDS_CAP, LDS_CAP + 1} <= set(t.tolist())
    staged = t <= LDS_CAP
    assert {1, 2, 3} <= set((t[staged] % 4).tolist()), "the scalar tail of the 16-byte copy"
    assert staged[0] and not staged[1] and not staged[2] and staged[3], "staged -> direct and direct -> staged in one workgroup"
    assert not staged[7] and staged[8] and staged[9] and not staged[10], "staged tiles between over-capacity ones"
    # rows of a staged tile beyond one trip of 8 gathers, with and without a partial last trip
    rows_staged = lengths[np.repeat(staged, 256)[:3001]]
    long = rows_staged[rows_staged > 8]
    assert (long % 8 == 0).any() and (long % 8 != 0).any()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9])
@pytest.mark.parametrize("name", ["tiles", "V1", "V63", "V64", "V65", "V255", "V256", "V257", "V4001"])
def test_spmv_on_irregular_rows(dev, name, k):
    from largesteps import _native
    from largesteps.parameterize import to_differential
    M, A, lengths = _spmv_case(name, dev)
    V = lengths.shape[0]
    x = np.random.default_rng(100 + k).standard_normal((V, k)).astype(np.float32)
    xd = _t(x, dev)
    csr = _native.csr_of(M)
    assert np.array_equal(np.diff(csr.rowptr.cpu().numpy()), lengths), "the CSR side car has the requested rows"
    y0 = _native.spmv(csr, xd, 0)
    y1 = _native.spmv(csr, xd, 1)
    _assert_within_fma_bound(y0.cpu().numpy(), A, x, lengths, f"spmv variant 0, {name}, k={k}")
    _assert_within_fma_bound(y1.cpu().numpy(), A, x, lengths, f"spmv variant 1, {name}, k={k}")
    assert torch.equal(y0, y1), "the LDS-staged and the direct variant multiply in row order: the same bits"
    for variant, y in ((0, y0), (1, y1)):
        assert torch.equal(_raw_spmv(csr, xd, variant), y), "a second call gives the same bits, and every element is written"
    u = to_differential(M, xd)
    assert torch.equal(u, y0), "to_differential is the staged variant"
    if k == 1:
        assert torch.equal(to_differential(M, xd[:, 0].contiguous()), y0[:, 0])


@pytest.mark.parametrize("k", [1, 3, 5])
def test_to_differential_backward_through_long_columns(dev, k):
    """The gradient of u = A v is A^T g, the same kernel on the transposed side car. A is the transpose of the tiled matrix: unsymmetric,
    its COLUMNS are the irregular ones (lengths 0 .. 3000, tiles on both sides of LDS_CAP), so the backward product runs every branch."""
    from largesteps import _native
    from largesteps.parameterize import to_differential
    _, B, col_lengths = _spmv_case("tiles", dev)
    V = B.shape[0]
    A = B.T.tocsr().astype(np.float32)
    A.sort_indices()
    M = im.coo_of(A, dev)
    A = A.astype(np.float64)
    assert abs(A - A.T).max() > 0 and np.array_equal(np.diff(A.tocsc().indptr), col_lengths) and col_lengths.max() >= 300
    row_lengths = np.diff(A.indptr)
    rng = np.random.default_rng(k)
    v = rng.standard_normal((V, k)).astype(np.float32)
    g = rng.standard_normal((V, k)).astype(np.float32)
    vd = _t(v, dev).requires_grad_(True)
    u = to_differential(M, vd)
    (u * _t(g, dev)).sum().backward()
    assert not _native.is_symmetric(_native.csr_of(M), exact=True)
    _assert_within_fma_bound(u.detach().cpu().numpy(), A, v, row_lengths, f"forward of the transposed tiled matrix, k={k}")
    _assert_within_fma_bound(vd.grad.cpu().numpy(), A.T.tocsr(), g, col_lengths, f"backward (A^T g) over column lengths, k={k}")
    first = vd.grad.clone()
    vd.grad = None
    (to_differential(M, vd) * _t(g, dev)).sum().backward()
    assert torch.equal(vd.grad, first), "the same bits on a second backward pass"


# =====================================================================================================================================
# iterative solvers
# =====================================================================================================================================
_MESH = {}
_SYSTEM = {}

UNIFORM = dict(lambda_=10.0)
# cotangent weights: M = I + L_cot. The cotangent matrix is positive semi-definite as a quadratic form on any mesh without degenerate
# faces, but it is assembled in fp32 and the Delaunay sheet's hull has slivers (weights of ~3000): _system() therefore factorises the
# fp32-assembled M by a dense fp64 Cholesky and fails loudly if that does not succeed. It succeeds for the seeds used here
# (delaunay_sheet(4000, seed=0), delaunay_sheet(12000, seed=0)); pick another seed if a change of the generator breaks it.
COTAN = dict(lambda_=1.0, cotan=True)


def _mesh(name):
    if name not in _MESH:
        _MESH[name] = {"delaunay": lambda: im.delaunay_sheet(4000, seed=0), "planted": lambda: im.planted_plane(64)[:2],
                       "hub": lambda: im.hub_mesh(64, valences=(40, 300))[:2], "planted100": lambda: im.planted_plane(100)[:2],
                       "delaunay12k": lambda: im.delaunay_sheet(12000, seed=0)}[name]()
    return _MESH[name]


def _system(name, cot, dev):
    """(M, fp64 direct solver of the fp32-assembled M, fp64 scipy matrix); built once per module"""
    key = (name, cot)
    if key not in _SYSTEM:
        from largesteps.geometry import compute_matrix
        v, f = _mesh(name)
        M = compute_matrix(_t(v, dev), _t(f, dev), **(COTAN if cot else UNIFORM))
        idx, val = M.indices().cpu().numpy(), M.values().cpu().numpy()
        V = v.shape[0]
        lu = osv.DirectSolver(idx[0], idx[1], val, V)
        if cot and V <= 5000:
            np.linalg.cholesky(lu.A.toarray())           # LinAlgError: not positive definite -- see COTAN above
        _SYSTEM[key] = (M, lu, lu.A.tocsr())
    return _SYSTEM[key]


def _rhs(V, k, dev, seed=0):
    b = np.random.default_rng(1000 * seed + k).standard_normal((V, k)).astype(np.float32)
    return b, _t(b, dev)


def _solve_strictly(s, b):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return s.solve(b)


def _assert_solution(x, lu, b, what):
    x64 = lu.solve(b)
    err = np.abs(x.cpu().numpy().astype(np.float64) - x64).max() / np.abs(x64).max()
    print(f"[row kernels] {what}: forward error {err:.3e}")
    assert err <= TOL, f"{what}: ||x - x*||_inf = {err:.3e} ||x*||_inf"


def test_the_solver_meshes_reach_the_wide_branches():
    """The coverage the solver tests below rest on, asserted here so that a change of the helpers cannot lose it silently."""
    for name in ("delaunay", "planted", "hub"):
        v, f = _mesh(name)
        val = im.valence(v.shape[0], f)
        for widths, kernel in ((im.sell_widths(val + 1), "row_sell"), (im.sell_widths(val), "k_cheb_uniform")):
            assert (widths > 8).any(), f"{name}: no SELL slice wider than 8 for {kernel}"
            if name != "delaunay":
                assert (widths <= 8).any(), f"{name}: no SELL slice of width <= 8 for {kernel}"
        w = im.sell_widths(val + 1)
        assert ((w > 8) & (w % 4 != 0)).any(), f"{name}: the tail of row_sell's 4-way loop"
    w = im.sell_widths(im.valence(4000, _mesh("delaunay")[1]) + 1)
    assert ((w > 8) & (w % 4 == 0)).any() and (w >= 9).all()
    assert im.sell_widths(im.valence(_mesh("hub")[0].shape[0], _mesh("hub")[1])).max() == 300


@pytest.mark.parametrize("block", [0, 256, 512, 1024])
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("cot", [False, True])
@pytest.mark.parametrize("name", ["delaunay", "planted", "hub"])
def test_pcg_on_irregular_meshes(dev, name, cot, k, block):
    """k_init / k_spmv_dot / k_resnorm on row_sell's wide form"""
    from largesteps.solvers import PCGSolver
    M, lu, _ = _system(name, cot, dev)
    b, bd = _rhs(M.shape[0], k, dev)
    s = PCGSolver(M, rtol=1e-6)
    s.set_option("block", block)
    x = _solve_strictly(s, bd)
    assert s.last_info["method"] == "pcg" and s.last_info["converged"] and 5 < s.last_info["iterations"] < 1000
    _assert_solution(x, lu, b, f"PCG {name} cot={cot} k={k} block={block}")
    assert torch.equal(_solve_strictly(s, bd), x), "a repeated solve gives the same bits"


@pytest.mark.parametrize("block", [0, 256, 512, 1024])
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("cot", [False, True])
@pytest.mark.parametrize("name", ["delaunay", "planted", "hub"])
def test_explicit_value_chebyshev_on_irregular_meshes(dev, monkeypatch, name, cot, k, block):
    """k_cheb on row_sell's wide form (LARGESTEPS_EXPLICIT_VALUES keeps the uniform matrices on the {col, val} kernel)"""
    from largesteps.solvers import PCGSolver
    monkeypatch.setenv("LARGESTEPS_EXPLICIT_VALUES", "1")
    M, lu, _ = _system(name, cot, dev)
    b, bd = _rhs(M.shape[0], k, dev)
    s = PCGSolver(M, rtol=1e-6, chebyshev=True, chebyshev_cap=1000000)      # (a hub or a sliver loosens the enclosure: no cap here)
    assert s.chebyshev and not s.implicit_values and s.patch_plan is None
    s.set_option("block", block)
    x = _solve_strictly(s, bd)
    assert s.last_info["method"] == "chebyshev" and s.last_info["converged"]
    assert s.last_info["iterations"] == s.chebyshev_iterations
    _assert_solution(x, lu, b, f"Chebyshev (explicit values) {name} cot={cot} k={k} block={block}")
    assert torch.equal(_solve_strictly(s, bd), x), "a repeated solve gives the same bits"


@pytest.mark.parametrize("block", [0, 256, 512, 1024])
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("name", ["delaunay", "planted", "hub"])
def test_implicit_value_chebyshev_on_irregular_meshes(dev, monkeypatch, name, k, block):
    """k_cheb_uniform on slices wider than 8 (neighbour ids only, the diagonal not counted)"""
    from largesteps.solvers import PCGSolver
    monkeypatch.delenv("LARGESTEPS_EXPLICIT_VALUES", raising=False)
    M, lu, _ = _system(name, False, dev)
    b, bd = _rhs(M.shape[0], k, dev)
    s = PCGSolver(M, rtol=1e-6, chebyshev=True, chebyshev_cap=1000000)
    assert s.chebyshev and s.implicit_values and s.patch_plan is None
    s.set_option("block", block)
    x = _solve_strictly(s, bd)
    assert s.last_info["method"] == "chebyshev" and s.last_info["converged"]
    _assert_solution(x, lu, b, f"Chebyshev (implicit values) {name} k={k} block={block}")
    assert torch.equal(_solve_strictly(s, bd), x), "a repeated solve gives the same bits"


@pytest.mark.parametrize("name", ["delaunay", "planted", "hub"])
def test_the_enclosure_contains_the_spectrum_on_irregular_meshes(dev, name):
    """[lmin, lmax] of ls_solver_spectrum contains spec(D^-1/2 M D^-1/2) (dense fp64 eigenvalues): a vertex of valence 300 makes the
    enclosure loose, never wrong. The default cap then prefers PCG on the hub mesh -- which is why the tests above pass the cap."""
    from largesteps import _native
    from largesteps.solvers import PCGSolver
    M, lu, A = _system(name, False, dev)
    s = PCGSolver(M, rtol=1e-6, chebyshev=True, chebyshev_cap=1000000)
    assert s.chebyshev and s.implicit_values
    lo, hi = ctypes.c_double(), ctypes.c_double()
    _native.check(_native.lib().ls_solver_spectrum(s._handle, ctypes.byref(lo), ctypes.byref(hi)))
    D = A.toarray()
    d = np.diag(D)
    ev = np.linalg.eigvalsh(D / np.sqrt(np.outer(d, d)))
    assert lo.value <= ev.min() * (1 + 1e-6) and ev.max() <= hi.value * (1 + 1e-6)
    if name == "hub":
        assert d.max() == 1.0 + 10.0 * 300 and not PCGSolver(M, rtol=1e-6, chebyshev=True).chebyshev


@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("name,patch_cfg", [("planted100", "128,3,2000,2"), ("planted100", "256,4,2000,2"), ("delaunay12k", "128,3,2000,2")])
def test_patch_kernel_on_every_width_class(dev, monkeypatch, name, patch_cfg, k):
    """k_patch_cheb: ids in registers for W <= 6, == 7, == 8, re-read for W > 8 -- all four in the one plan of the planted plane; the
    Delaunay sheet's patches are all wider than 8. Patch kernel and one-step kernel solve the same system, both held to fp64."""
    from largesteps.solvers import PCGSolver
    monkeypatch.delenv("LARGESTEPS_EXPLICIT_VALUES", raising=False)
    monkeypatch.delenv("LARGESTEPS_NO_PATCHES", raising=False)
    monkeypatch.setenv("LARGESTEPS_PATCH", patch_cfg)
    M, lu, _ = _system(name, False, dev)
    b, bd = _rhs(M.shape[0], k, dev)
    s = PCGSolver(M, rtol=1e-6, chebyshev=True, chebyshev_cap=1000000, patch_min_vertices=1000)
    assert s.chebyshev and s.implicit_values and s.patch_plan is not None and s.patch_plan.n_patches >= 32
    classes = im.width_classes(s.patch_plan.table[:, 4])
    assert classes == ({"<=6", "7", "8", ">8"} if name == "planted100" else {">8"}), f"patch widths {np.bincount(s.patch_plan.table[:, 4])}"
    x = _solve_strictly(s, bd)
    assert s.last_info["method"] == "chebyshev" and s.last_info["converged"]
    _assert_solution(x, lu, b, f"patch kernel {name} {patch_cfg} k={k}")
    assert torch.equal(_solve_strictly(s, bd), x), "a repeated solve gives the same bits"
    s.set_option("patch", 0)                       # the same handle, one-step kernel
    y = _solve_strictly(s, bd)
    assert s.last_info["method"] == "chebyshev" and s.last_info["converged"]
    _assert_solution(y, lu, b, f"one-step kernel {name} k={k}")


def test_from_differential_on_a_delaunay_mesh_iterative_and_direct(dev, monkeypatch):
    """The public entry point on irregular rows: 'Cholesky' through the iteration (LARGESTEPS_NO_DIRECT) and through the default
    direct solver, forward and gradient against fp64."""
    from largesteps.geometry import compute_matrix
    from largesteps.parameterize import from_differential
    from largesteps.solvers import CholeskySolver
    v, f = _mesh("delaunay")
    b, _ = _rhs(v.shape[0], 3, dev, seed=2)
    w, wd = _rhs(v.shape[0], 3, dev, seed=3)
    for no_direct in (True, False):
        if no_direct:
            monkeypatch.setenv("LARGESTEPS_NO_DIRECT", "1")
        else:
            monkeypatch.delenv("LARGESTEPS_NO_DIRECT", raising=False)
        M = compute_matrix(_t(v, dev), _t(f, dev), **UNIFORM)            # a matrix of its own: from_differential caches its solver per matrix
        idx, val = M.indices().cpu().numpy(), M.values().cpu().numpy()
        lu = osv.DirectSolver(idx[0], idx[1], val, v.shape[0])
        u = _t(b, dev).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert CholeskySolver(M).method == ("iterative" if no_direct else "nested-dissection")
            x = from_differential(M, u, "Cholesky")
            (x * wd).sum().backward()
        _assert_solution(x.detach(), lu, b, f"from_differential forward, no_direct={no_direct}")
        _assert_solution(u.grad, lu, w, f"from_differential gradient, no_direct={no_direct}")
