"""
The iterative solvers' stopping rule, caps and breakdown reports (-m gpu), against tests/stopping_statement.py.

PCGSolver promises: a column is converged when ||r||_2 <= max(rtol ||b||_2, atol), per column; a converged column is frozen while the
others go on; max_iter bounds the work; a breakdown is an error, not an answer. csrc/pcg.hip spreads that over k_init_scal (thr2, mask,
stop_iter), k_update (alpha = 0 for a masked column, the p.Ap <= 0 report), k_direction (next mask, the non-finite report, stop_iter), the
early return of every kernel, the look-ahead of solve_impl, the a-priori count and the acceptance test of solve_cheb, and
PCGSolver._solve_block. Cases a-i below are the ones of that list.

Mesh: icosphere(20), 4002 vertices (a ragged last tile and SELL slice), radial noise 0.05, seed 2; the cotangent matrix (lambda_=0,
alpha=0.9) and the uniform one (lambda_=25). All fp64 work is numpy / scipy.

MARGINS. "true residual <= threshold x margin": the recurrence residual of an fp32 run drifts from the true one, so the true residual of
a converged fp32 solve may exceed the threshold. How far is measured on the fp32 STATEMENT of the same case (never on the kernel): margin
= 2 x the largest (true fp64 residual / threshold) the statement reaches; the factor 2 covers the kernels' fused multiply-adds and
summation order. A case whose statement exceeds 4 x its threshold is below the fp32 floor and is refused by _margin(). Both ratios are
printed under -s; the values seen on the MI355X are in docs/measurements.md.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import stopping_statement as ss
from oracle import solve as osv

pytestmark = pytest.mark.gpu

KINDS = {"cot": dict(lambda_=0.0, alpha=0.9, cotan=True), "uniform": dict(lambda_=25.0)}
SCALES = np.array([1.0, 1e-6, 1e6, 0.0])
TOL = 1e-4              # forward error of every solve path against the fp64 direct solve


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()          # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_SYS = {}
_STMT = {}


def _system(kind, dev):
    """(M on the device, fp64 scipy matrix of the fp32-assembled M, fp64 direct solver); built once per module"""
    if kind not in _SYS:
        from largesteps import synthetic
        from largesteps.geometry import compute_matrix
        v, f = synthetic.icosphere(20)
        v = synthetic.perturb(v, radial=0.05, seed=2)
        M = compute_matrix(_t(v, dev), _t(f, dev), **KINDS[kind])
        idx, val = M.indices().cpu().numpy(), M.values().cpu().numpy()
        _SYS[kind] = (M, ss.system_matrix(idx[0], idx[1], val, v.shape[0]), osv.DirectSolver(idx[0], idx[1], val, v.shape[0]))
    return _SYS[kind]


def _normal(V, k, seed=0):
    return np.random.default_rng(1000 * seed + k).standard_normal((V, k)).astype(np.float32)


def _smooth(A):
    return (A @ np.ones(A.shape[0])).astype(np.float32)


def _stmt(key, A, b, **kw):
    """the statement of one case, computed once (key names the matrix and b) and left unchanged"""
    key = (key, tuple(sorted((k, str(v)) for k, v in kw.items() if k != "x0")), "x0" in kw)
    if key not in _STMT:
        _STMT[key] = ss.pcg(A, b, **kw)
    return _STMT[key]


def _margin(st32, what):
    """2 x the largest true residual / threshold of the fp32 statement; refuses a case below the fp32 floor"""
    on = st32.thr > 0
    worst = float((st32.true_rnorm[on] / st32.thr[on]).max()) if on.any() else 0.0
    assert worst <= 4.0, f"{what}: the fp32 statement is at {worst:.2f} x its threshold: below the fp32 floor, not a case for this suite"
    return 2.0 * worst, worst


def _assert_residuals(A, x, b, thr, margin, worst32, what):
    true = ss.true_residual(A, x.cpu().numpy(), b)
    on = thr > 0
    ratio = float((true[on] / thr[on]).max()) if on.any() else 0.0
    print(f"[stopping] {what}: true residual / threshold: kernel {ratio:.3f}, fp32 statement {worst32:.3f}, bound {margin:.3f}")
    assert (true[on] <= margin * thr[on]).all(), f"{what}: true residual / threshold = {true[on] / thr[on]} > {margin:.3f}"
    return ratio


def _solve(s, b, expect_warning=None, **kw):
    """s.solve(b) with no warning at all, or with exactly the expected ones (in order; "a|b": the message holds a and b)"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        x = s.solve(b, **kw)
    got = [str(m.message) for m in w if issubclass(m.category, RuntimeWarning)]
    want = list(expect_warning or [])
    assert len(got) == len(want) and all(part in g for t, g in zip(want, got) for part in t.split("|")), f"warnings {got}, expected {want}"
    return x


def _spectrum(s):
    from largesteps import _native
    lo, hi = ctypes.c_double(), ctypes.c_double()
    _native.check(_native.lib().ls_solver_spectrum(s._handle, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def _assert_forward(x, lu, b, what):
    x64 = lu.solve(b)
    err = np.abs(x.cpu().numpy().astype(np.float64) - x64).max() / np.abs(x64).max()
    print(f"[stopping] {what}: forward error {err:.3e}")
    assert err <= TOL, f"{what}: ||x - x*||_inf = {err:.3e} ||x*||_inf"


# =====================================================================================================================================
# a. per-column thresholds
# =====================================================================================================================================
@pytest.mark.parametrize("rtol", [1e-3, 1e-6])
@pytest.mark.parametrize("cols", [(0, 1, 2, 3), (0, 1, 2), (1, 3, 2), (1, 2), (3, 0)])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_a_every_column_has_its_own_threshold(dev, kind, cols, rtol):
    """Columns scaled by 1, 1e-6, 1e6 and 0: each is held to rtol x ITS norm. A threshold shared among the columns (the largest norm's) would
    stop the 1e-6 column at once, twelve orders of magnitude short, and the count would be a few iterations instead of the statement's."""
    from largesteps.solvers import PCGSolver
    M, A, _ = _system(kind, dev)
    b = (_normal(A.shape[0], 4) * SCALES).astype(np.float32)[:, list(cols)]
    st32 = _stmt((kind, "scaled", cols), A, b, rtol=rtol, dtype=np.float32)
    margin, worst32 = _margin(st32, f"a {kind} {cols} rtol={rtol}")
    s = PCGSolver(M, rtol=rtol, chebyshev=False)
    x = _solve(s, _t(b, dev))
    info = s.last_info
    thr = ss.thresholds(b, rtol, 0.0)
    assert info["method"] == "pcg" and info["converged"]
    np.testing.assert_allclose(info["bnorm"], np.linalg.norm(b.astype(np.float64), axis=0), rtol=1e-6)
    assert (np.array(info["rnorm"]) <= thr * (1 + 1e-12)).all(), f"rnorm {info['rnorm']} thr {thr}"
    for j, c in enumerate(cols):
        if SCALES[c] == 0.0:
            assert float(x[:, j].abs().max()) == 0.0 and info["rnorm"][j] == 0.0 and info["bnorm"][j] == 0.0
    _assert_residuals(A, x, b, thr, margin, worst32, f"a {kind} cols={cols} rtol={rtol}")
    print(f"[stopping] a {kind} cols={cols} rtol={rtol}: iterations kernel {info['iterations']}, fp32 statement {st32.iterations}")
    assert abs(info["iterations"] - st32.iterations) <= 2


# =====================================================================================================================================
# b. freeze
# =====================================================================================================================================
_ALONE = {}


def _alone(kind, name, col, dev, rtol):
    """(x, last_info) of the k = 1 solve of one column; computed once"""
    from largesteps.solvers import PCGSolver
    if (kind, name) not in _ALONE:
        s = PCGSolver(_system(kind, dev)[0], rtol=rtol, chebyshev=False)
        x = _solve(s, _t(col[:, None], dev))
        _ALONE[(kind, name)] = (x[:, 0].clone(), dict(s.last_info))
    return _ALONE[(kind, name)]


@pytest.mark.parametrize("pos", ["first", "last"])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_b_a_converged_column_is_frozen_while_the_others_go_on(dev, k, pos, kind="uniform"):
    """M 1 (smooth: a third of the iterations) next to random columns, the smooth one in column 0 or k - 1. The uniform matrix only: under the
    cotangent matrix's Jacobi preconditioner M 1 needs as many iterations as a random column (statement: 41 against 40), no freeze case. At rtol
    = 1e-3 every further iteration would move the smooth column by about 1e-3 of its size and shrink its residual by orders of magnitude:
    both are held to 1e-6 / 1e-4 of the k = 1 solve of that column alone (not to its bits: the reduction order differs with K)."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-3
    M, A, _ = _system(kind, dev)
    V = A.shape[0]
    rnd = _normal(V, 3, seed=5)
    at = 0 if pos == "first" else k - 1
    cols, names = [], []
    for j in range(k):
        if j == at:
            cols.append(_smooth(A)); names.append("smooth")
        else:
            n = len([t for t in names if t != "smooth"])
            cols.append(rnd[:, n]); names.append(f"rnd{n}")
    b = np.stack(cols, 1)
    x_s, info_s = _alone(kind, "smooth", b[:, at], dev, rtol)
    slow = max(_alone(kind, names[j], b[:, j], dev, rtol)[1]["iterations"] for j in range(k) if j != at)
    st = _stmt((kind, "freeze", k, pos), A, b, rtol=rtol, dtype=np.float32)
    assert st.freeze[at] + 10 < min(st.freeze[j] for j in range(k) if j != at), "the case needs a column that stops well before the others"
    s = PCGSolver(M, rtol=rtol, chebyshev=False)
    x = _solve(s, _t(b, dev))
    info = s.last_info
    print(f"[stopping] b {kind} k={k} {pos}: iterations {info['iterations']} (slowest column alone {slow}, smooth alone {info_s['iterations']}, "
          f"statement freeze {st.freeze.tolist()})")
    assert info["converged"] and abs(info["iterations"] - slow) <= 2
    assert abs(info_s["iterations"] - st.freeze[at]) <= 2
    d = float((x[:, at] - x_s).abs().max()) / float(x_s.abs().max())
    assert d <= 1e-6, f"the frozen column moved: {d:.3e} of ||x||_inf"
    assert abs(info["rnorm"][at] - info_s["rnorm"][0]) <= 1e-4 * info_s["rnorm"][0], (info["rnorm"][at], info_s["rnorm"][0])
    assert info["rnorm"][at] > 1e-2 * rtol * info["bnorm"][at], "the residual norm of the frozen column is the one at its freeze"


# =====================================================================================================================================
# c. look-ahead changes nothing
# =====================================================================================================================================
@pytest.mark.parametrize("block", [0, 256])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_c_chunk_length_and_check_every_do_not_change_the_answer(dev, kind, block):
    """The host enqueues whole chunks ahead of what it has looked at; kernels past stop_iter must be no-ops: the same bits and the same
    count for check_every = 1, 16, 4096 and for a second solve on the same handle (whose first chunk is last_iters long)."""
    from largesteps.solvers import PCGSolver
    M, A, _ = _system(kind, dev)
    V = A.shape[0]
    rnd = _normal(V, 2, seed=6)
    b = _t(np.stack([rnd[:, 0], _smooth(A), rnd[:, 1] * np.float32(1e-6)], 1), dev)      # three different freeze iterations
    ref = None
    for every in (16, 1, 4096):
        s = PCGSolver(M, rtol=1e-6, chebyshev=False)
        s.set_option("block", block)
        s.set_option("check_every", every)
        x = _solve(s, b)
        first = dict(s.last_info)
        assert first["converged"] and first["iterations"] > 20
        x2 = _solve(s, b)
        assert torch.equal(x2, x) and s.last_info == first, f"check_every={every}: the second solve on the handle differs"
        if ref is None:
            ref = (x, first)
        assert torch.equal(x, ref[0]), f"check_every={every} changes the answer"
        assert first == ref[1], f"check_every={every}: {first} != {ref[1]}"


# =====================================================================================================================================
# d. caps
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_d_max_iter_stops_after_exactly_that_many_steps(dev, kind):
    """max_iter = needed - 5: a warning, converged False, iterations == max_iter and the iterate of exactly that many steps. The kernel and
    the fp32 statement are two fp32 runs of the same m steps; e = ||x32 - x64||_2 is what the statement's rounding moves the m-step iterate
    by, and the kernel is held to 2 e (the margin rule of this file), which must also be < 10 % of the distance to the neighbouring iterates
    (m - 1 and m + 1 steps) for the assertion to tell an off-by-one."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-3
    M, A, _ = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=7)
    bd = _t(b, dev)
    s = PCGSolver(M, rtol=rtol, chebyshev=False)
    x_full = _solve(s, bd)
    need = s.last_info["iterations"]
    assert s.last_info["converged"] and need > 10
    m = need - 5
    st32 = _stmt((kind, "cap", m), A, b, rtol=rtol, max_iter=m, dtype=np.float32)
    st64 = _stmt((kind, "cap", m), A, b, rtol=rtol, max_iter=m)
    assert st32.iterations == m and st64.iterations == m and not st64.converged.all() and not st32.converged.all()
    e = np.linalg.norm(st32.x.astype(np.float64) - st64.x)
    near = min(np.linalg.norm(ss.pcg(A, b, rtol=rtol, max_iter=m + d).x - st64.x) for d in (-1, 1))
    assert 2 * e < 0.1 * near, "the bound does not separate m steps from m +- 1"
    capped = PCGSolver(M, rtol=rtol, max_iter=m, chebyshev=False)
    x = _solve(capped, bd, expect_warning=["not converged"])
    info = capped.last_info
    assert info["method"] == "pcg" and not info["converged"] and info["iterations"] == m
    got = np.linalg.norm(x.cpu().numpy().astype(np.float64) - st64.x)
    print(f"[stopping] d {kind}: needed {need}, capped at {m}: ||x - x64_m||_2 kernel {got:.3e}, fp32 statement {e:.3e}, next iterate {near:.3e}")
    assert got <= 2 * e
    assert (np.array(info["rnorm"]) > ss.thresholds(b, rtol, 0.0)).any()
    # exactly enough: converged, no warning, the uncapped answer
    enough = PCGSolver(M, rtol=rtol, max_iter=need, chebyshev=False)
    assert torch.equal(_solve(enough, bd), x_full) and enough.last_info["converged"] and enough.last_info["iterations"] == need
    # none at all: the start is returned
    zero = PCGSolver(M, rtol=rtol, max_iter=0, chebyshev=False, warm_start=True)
    x0 = _solve(zero, bd, expect_warning=["not converged"])
    assert float(x0.abs().max()) == 0.0 and not zero.last_info["converged"] and zero.last_info["iterations"] == 0
    guess = _t(_normal(A.shape[0], 3, seed=8), dev)
    zero.guess_fwd = guess.clone()
    xg = _solve(zero, bd, expect_warning=["not converged"])
    assert torch.equal(xg, guess) and not zero.last_info["converged"] and zero.last_info["iterations"] == 0


@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_d_a_capped_chebyshev_run_is_refused_and_pcg_answers(dev, kind):
    """max_iter below the a-priori Chebyshev count: the (capped) Chebyshev iterate is not returned; the Python layer warns, falls back, and
    the result is PCG's under the same cap."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-6
    M, A, lu = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=9)
    probe = PCGSolver(M, rtol=rtol, chebyshev=True)
    assert probe.chebyshev
    n_cheb = ss.chebyshev_count(*_spectrum(probe), rtol=rtol)
    assert probe.chebyshev_iterations == n_cheb
    st32 = _stmt((kind, "cheb-cap"), A, b, rtol=rtol, dtype=np.float32)
    m = n_cheb - 1
    s = PCGSolver(M, rtol=rtol, max_iter=m, chebyshev=True)
    pcg_fits = st32.iterations + 2 <= m
    x = _solve(s, _t(b, dev), expect_warning=["exceed max_iter|falling back to PCG"] + ([] if pcg_fits else ["not converged"]))
    info = s.last_info
    print(f"[stopping] d {kind}: Chebyshev count {n_cheb}, cap {m}, PCG statement {st32.iterations}, PCG ran {info['iterations']}")
    assert info["method"] == "pcg" and info["iterations"] <= m
    thr = ss.thresholds(b, rtol, 0.0)
    assert info["converged"] == bool((np.array(info["rnorm"]) <= thr * (1 + 1e-12)).all())
    if pcg_fits:
        assert info["converged"]
        _assert_forward(x, lu, b, f"d {kind}: PCG after a refused Chebyshev run")


# =====================================================================================================================================
# e. atol only, and ConjugateGradientSolver
# =====================================================================================================================================
@pytest.mark.parametrize("chebyshev", [False, True])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_e_absolute_tolerance_alone(dev, kind, chebyshev):
    """rtol = 0, atol = 1e-3 ||b_0||: the threshold is atol for every column; on the Chebyshev path the count is the statement's at the
    enclosure the handle reports (cold start: ||r0|| = ||b||)."""
    from largesteps.solvers import PCGSolver
    M, A, _ = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=10)
    atol = 1e-3 * float(np.linalg.norm(b[:, 0].astype(np.float64)))
    st32 = _stmt((kind, "atol"), A, b, rtol=0.0, atol=atol, dtype=np.float32)
    margin, worst32 = _margin(st32, f"e {kind} atol")
    s = PCGSolver(M, rtol=0.0, atol=atol, chebyshev=chebyshev)
    assert s.chebyshev == chebyshev
    x = _solve(s, _t(b, dev))
    info = s.last_info
    thr = np.full(3, atol)
    assert info["converged"] and info["method"] == ("chebyshev" if chebyshev else "pcg")
    assert (np.array(info["rnorm"]) <= thr * (1 + 1e-12)).all()
    _assert_residuals(A, x, b, thr, margin, worst32, f"e {kind} atol chebyshev={chebyshev}")
    if chebyshev:
        assert info["iterations"] == ss.chebyshev_count(*_spectrum(s), thr=thr, r0=np.linalg.norm(b.astype(np.float64), axis=0))
    else:
        assert abs(info["iterations"] - st32.iterations) <= 2


@pytest.mark.parametrize("chebyshev", [False, True])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_e_conjugate_gradient_solver_rule_and_warm_starts(dev, kind, chebyshev):
    """ConjugateGradientSolver: ||r|| <= 1e-5 absolute, warm started, forward and backward guesses kept apart. b has unit-norm columns, so
    the threshold is 1e-5 ||b||: above the fp32 floor (checked on the fp32 statement first)."""
    from largesteps.solvers import ConjugateGradientSolver
    M, A, _ = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=11)
    b = (b / np.linalg.norm(b.astype(np.float64), axis=0)).astype(np.float32)
    st32 = _stmt((kind, "cg"), A, b, rtol=0.0, atol=1e-5, dtype=np.float32)
    margin, worst32 = _margin(st32, f"e {kind} CG")
    thr = np.full(3, 1e-5)
    s = ConjugateGradientSolver(M, chebyshev=chebyshev)
    assert s.chebyshev == chebyshev and s.warm_start and s.rtol == 0.0 and s.atol == 1e-5
    bd = _t(b, dev)
    x = _solve(s, bd)
    cold = dict(s.last_info)
    assert cold["converged"] and cold["method"] == ("chebyshev" if chebyshev else "pcg")
    _assert_residuals(A, x, b, thr, margin, worst32, f"e {kind} CG cold chebyshev={chebyshev}")
    n_cold = ss.chebyshev_count(*_spectrum(s), thr=thr, r0=np.linalg.norm(b.astype(np.float64), axis=0)) if chebyshev else st32.iterations
    assert (cold["iterations"] == n_cold) if chebyshev else (abs(cold["iterations"] - n_cold) <= 2)
    assert s.guess_fwd is x and s.guess_bwd is None
    # warm: 1.01 b from the solution of b
    b2 = (b * np.float32(1.01)).astype(np.float32)
    x_prev = x.clone()
    x2 = _solve(s, _t(b2, dev))
    warm = dict(s.last_info)
    st_warm = _stmt((kind, "cg-warm"), A, b2, x0=st32.x, rtol=0.0, atol=1e-5, dtype=np.float32)
    m2, w2 = _margin(st_warm, f"e {kind} CG warm")
    print(f"[stopping] e {kind} CG chebyshev={chebyshev}: iterations cold {cold['iterations']}, warm {warm['iterations']}")
    assert warm["converged"] and warm["iterations"] < cold["iterations"]
    _assert_residuals(A, x2, b2, thr, m2, w2, f"e {kind} CG warm chebyshev={chebyshev}")
    assert s.guess_fwd is x2 and s.guess_bwd is None
    # backward after forward: its own guess, i.e. none yet -- a cold start
    g = _solve(s, bd, backward=True)
    assert s.last_info["iterations"] == cold["iterations"], "the first backward solve starts cold"
    assert torch.equal(g, x_prev), "and is the cold forward solve of the same b, bit for bit"
    assert s.guess_bwd is g and s.guess_fwd is x2


# =====================================================================================================================================
# f. mixed starting distances on the Chebyshev path
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_f_chebyshev_count_follows_the_column_furthest_from_its_threshold(dev, kind):
    """Warm start, column 0 at the solution (inside its threshold), column 1 at zero: the count is what column 1 needs."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-3
    M, A, lu = _system(kind, dev)
    b = _normal(A.shape[0], 2, seed=12)
    guess = np.zeros_like(b)
    guess[:, 0] = lu.solve(b[:, :1])[:, 0].astype(np.float32)
    thr = ss.thresholds(b, rtol, 0.0)
    r0 = ss.true_residual(A, guess, b)
    assert r0[0] < 0.1 * thr[0] and abs(r0[1] - np.linalg.norm(b[:, 1].astype(np.float64))) <= 1e-12 * r0[1]
    st32 = _stmt((kind, "mixed"), A, b, x0=guess, rtol=rtol, dtype=np.float32)
    margin, worst32 = _margin(st32, f"f {kind}")
    assert st32.freeze[0] == 0
    s = PCGSolver(M, rtol=rtol, chebyshev=True, warm_start=True)
    assert s.chebyshev
    s.guess_fwd = _t(guess, dev)
    x = _solve(s, _t(b, dev))
    info = s.last_info
    n = ss.chebyshev_count(*_spectrum(s), thr=thr, r0=r0)
    assert n == ss.chebyshev_count(*_spectrum(s), rtol=rtol) > 0
    assert info["method"] == "chebyshev" and info["converged"] and info["iterations"] == n
    _assert_residuals(A, x, b, thr, margin, worst32, f"f {kind} mixed start")


@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_f_zero_column_with_a_nonzero_guess(dev, kind):
    """b has an all-zero column and the warm start is not zero there: the threshold is 0 and the rule cannot be met (test_solver_geometries_
    and_widths notes the same). What the code does, with max_iter = 200: the Chebyshev count for a reduction to 0 (asked as 1e-30) is
    above any sensible cap, so the capped Chebyshev run is refused; PCG then starts from the guess, freezes the other columns when they meet
    their thresholds and iterates the zero column until max_iter -- its recurrence residual shrinks every iteration but reaches exactly 0
    only by underflow, hundreds of iterations later. The call warns twice, returns, and reports converged = False: max_iter Chebyshev steps
    plus max_iter PCG iterations on every such solve (docs/measurements.md)."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-3
    M, A, _ = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=13)
    b[:, 1] = 0.0
    thr = ss.thresholds(b, rtol, 0.0)
    s = PCGSolver(M, rtol=rtol, max_iter=200, chebyshev=True, warm_start=True)
    guess = _normal(A.shape[0], 3, seed=14)
    s.guess_fwd = _t(guess, dev)
    x = _solve(s, _t(b, dev), expect_warning=["exceed max_iter|falling back to PCG", "not converged"])
    info = s.last_info
    rn = np.array(info["rnorm"])
    print(f"[stopping] f {kind} zero column, nonzero guess: method {info['method']}, iterations {info['iterations']}, rnorm {rn}, thr {thr}")
    assert info["method"] == "pcg" and info["iterations"] == 200
    assert rn[1] > thr[1] == 0.0 and not info["converged"], "no claim of convergence for a column above its threshold"
    assert (rn[[0, 2]] <= thr[[0, 2]] * (1 + 1e-12)).all()
    st32 = _stmt((kind, "zero-col"), A, b[:, [0, 2]], x0=guess[:, [0, 2]], rtol=rtol, dtype=np.float32)
    margin, worst32 = _margin(st32, f"f {kind} zero column")
    _assert_residuals(A, x[:, [0, 2]], b[:, [0, 2]], thr[[0, 2]], margin, worst32, f"f {kind} the other columns")


# =====================================================================================================================================
# g. more than four columns
# =====================================================================================================================================
@pytest.mark.parametrize("k", [5, 7, 9])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_g_wide_right_hand_sides_are_solved_in_blocks(dev, kind, k):
    """k > 4: blocks of <= 4 columns, every block to its own thresholds, the warm-start guess kept in full and used block by block."""
    from largesteps.solvers import PCGSolver
    rtol = 1e-3
    M, A, lu = _system(kind, dev)
    scales = np.array([1.0, 1e-6, 1e6, 3.0, 1e-3, 1e3, 1.0, 1e-6, 1e6])[:k]
    b = (_normal(A.shape[0], k, seed=15) * scales).astype(np.float32)
    st32 = _stmt((kind, "wide", k), A, b, rtol=rtol, dtype=np.float32)      # the columns are independent: one statement serves every block
    margin, worst32 = _margin(st32, f"g {kind} k={k}")
    thr = ss.thresholds(b, rtol, 0.0)
    s = PCGSolver(M, rtol=rtol, chebyshev=False, warm_start=True)
    bd = _t(b, dev)
    x = _solve(s, bd)
    last = k - 4 * ((k - 1) // 4)
    assert s.last_info["converged"] and len(s.last_info["rnorm"]) == last, "last_info is the last block's"
    assert (np.array(s.last_info["rnorm"]) <= thr[k - last:] * (1 + 1e-12)).all()
    assert abs(s.last_info["iterations"] - st32.freeze[k - last:].max()) <= 2
    _assert_residuals(A, x, b, thr, margin, worst32, f"g {kind} k={k}")
    assert s.guess_fwd is x and tuple(s.guess_fwd.shape) == (A.shape[0], k)
    # the exact solution as the guess: every block is converged at once
    exact = lu.solve(b).astype(np.float32)
    s.guess_fwd = _t(exact, dev)
    x2 = _solve(s, bd)
    assert s.last_info["converged"] and s.last_info["iterations"] <= 10
    _assert_residuals(A, x2, b, thr, margin, worst32, f"g {kind} k={k} from the exact guess")
    assert tuple(s.guess_fwd.shape) == (A.shape[0], k)


# =====================================================================================================================================
# h. breakdown reports
# =====================================================================================================================================
@pytest.mark.parametrize("col", ["first", "last"])
@pytest.mark.parametrize("row", ["first", "last"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_h_non_finite_right_hand_side_is_an_error_and_the_handle_survives(dev, value, row, col):
    """One inf / nan in b, in the first or the last row (the ragged tile) and the first or the last column: RuntimeError 'non-finite', no
    answer; the same handle then solves a good right-hand side correctly. (An error return: the kernels compute with the values and set
    a flag.)"""
    from largesteps.solvers import PCGSolver
    k = 3
    M, A, lu = _system("cot", dev)
    V = A.shape[0]
    good = _normal(V, k, seed=16)
    bad = good.copy()
    bad[0 if row == "first" else V - 1, 0 if col == "first" else k - 1] = value
    s = PCGSolver(M, rtol=1e-6, chebyshev=False)
    with pytest.raises(RuntimeError, match="non-finite"):
        s.solve(_t(bad, dev))
    assert not s.last_info["converged"] and s.last_info["iterations"] == 0
    x = _solve(s, _t(good, dev))
    assert s.last_info["converged"]
    _assert_forward(x, lu, good, f"h after {value} at row {row}, column {col}")


def test_h_indefinite_matrix_is_reported_not_solved(dev):
    """Foreign matrices made from the cotangent matrix. Its negative, -M, has a negative diagonal: the Jacobi preconditioner does not exist
    and the constructor refuses it (ValueError, 'not SPD') before any iteration. To reach the solve-time report the diagonal has to stay
    positive: M - c I with 0.1 = lambda_min(M) < c < min M_ii is indefinite (M 1 = 0.1 1 for alpha = 0.9), and CG's p.Ap <= 0 must come
    back as RuntimeError 'not positive definite', never as an answer."""
    from largesteps.solvers import PCGSolver
    M, A, _ = _system("cot", dev)
    V = A.shape[0]
    idx, val = M.indices(), M.values()
    neg = torch.sparse_coo_tensor(idx, -val, M.shape).coalesce()
    with pytest.raises(ValueError, match="not SPD"):
        PCGSolver(neg, rtol=1e-6)
    c = 0.5 * float(A.diagonal().min())
    assert c > 0.2 and abs((A @ np.ones(V)) - 0.1).max() < 1e-4
    shifted = torch.where(idx[0] == idx[1], val - c, val)
    Ms = torch.sparse_coo_tensor(idx, shifted, M.shape).coalesce()
    b = np.stack([np.ones(V, np.float32), _normal(V, 1, seed=17)[:, 0]], 1)
    for cols in ([0, 1], [1, 0], [0], [1]):
        s = PCGSolver(Ms, rtol=1e-6, max_iter=500)
        assert not s.chebyshev
        with pytest.raises(RuntimeError, match="not positive definite"):
            s.solve(_t(b[:, cols], dev))
        assert not s.last_info["converged"]


# =====================================================================================================================================
# i. Chebyshev refusal
# =====================================================================================================================================
@pytest.mark.parametrize("factor", [1000.0, 20.0])
@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_i_a_wrong_enclosure_is_refused_and_pcg_answers(dev, kind, factor):
    """a_min set too large on the handle: the enclosure no longer contains the spectrum. 1000 x puts a_min / max diag above the Gershgorin
    bound -- an empty enclosure, which solve_cheb used to turn into log(negative rate) = NaN iterations; it is now refused as a state
    error. 20 x leaves a valid interval that misses the low end of the spectrum: the a-priori count is too small, the iterate is far from
    converged, and the a-posteriori test max(thr2, floor2) must refuse it (the fp32 floor must not be so loose that it passes). Either way:
    one warning, PCG's answer, within 1e-4 of the fp64 direct solve."""
    from largesteps import _native
    from largesteps.solvers import PCGSolver
    M, A, lu = _system(kind, dev)
    b = _normal(A.shape[0], 3, seed=18)
    s = PCGSolver(M, rtol=1e-6, chebyshev=True)
    assert s.chebyshev
    lo, hi = _spectrum(s)
    _native.check(_native.lib().ls_solver_set_spectrum(s._handle, float(_native.csr_of(M).a_min) * factor))
    lo2, hi2 = _spectrum(s)
    assert abs(lo2 - factor * lo) <= 1e-12 * lo2 and hi2 == hi
    if factor == 1000.0:
        assert 0.98 * lo2 > hi * (1 + 1e-5), "the case: an empty enclosure"
        want = "spectral enclosure is empty"
    else:
        assert 0.98 * lo2 < hi, "the case: a valid interval that misses the low modes"
        want = "residual check failed"
    x = _solve(s, _t(b, dev), expect_warning=[want + "|falling back to PCG"])
    info = s.last_info
    print(f"[stopping] i {kind} a_min x {factor:g}: enclosure [{lo2:.4g}, {hi2:.4g}] (was [{lo:.4g}, {hi:.4g}]), PCG iterations {info['iterations']}")
    assert info["method"] == "pcg" and info["converged"] and 5 < info["iterations"] < 500
    _assert_forward(x, lu, b, f"i {kind} a_min x {factor:g}")
