"""
tests/stopping_statement.py held to the definition it states (no GPU): the rule ||r||_2 <= max(rtol ||b||_2, atol) per column, the freeze,
the cap, and the Chebyshev count formula. Matrices come from the oracle's assembly (fp32 values, as the solvers see them) on icosphere(4)
(162 vertices) and on the 4002-vertex sphere of the GPU tests.
"""
import math

import numpy as np
import pytest

import stopping_statement as ss
from largesteps import synthetic
from oracle import laplacian as ol, solve as osv

KINDS = {"cot": dict(lambda_=0.0, alpha=0.9, cotan=True), "uniform": dict(lambda_=25.0)}
SCALES = np.array([1.0, 1e-6, 1e6, 0.0])
_SYS = {}


def _system(n, kind):
    if (n, kind) not in _SYS:
        v, f = synthetic.icosphere(n)
        v = synthetic.perturb(v, radial=0.05, seed=2)
        r, c, val = ol.compute_matrix(v, f, **KINDS[kind])
        _SYS[(n, kind)] = (ss.system_matrix(r, c, val, v.shape[0]), (r, c, val))
    return _SYS[(n, kind)]


def _scaled_rhs(V, seed=0):
    return (np.random.default_rng(seed).standard_normal((V, 4)) * SCALES).astype(np.float32)


@pytest.mark.parametrize("kind", ["cot", "uniform"])
@pytest.mark.parametrize("n", [4, 20])
def test_fp64_freeze_iteration_is_the_first_that_meets_the_rule(n, kind):
    """True residual <= threshold at the freeze, > threshold one iteration earlier; the iterate of a frozen column stays; columns are
    independent (a multi-column solve is the single-column solves, freeze iterations included); the zero column freezes at 0 with x = 0."""
    A, _ = _system(n, kind)
    b = _scaled_rhs(A.shape[0])
    full = ss.pcg(A, b, rtol=1e-6)
    assert full.converged.all() and full.iterations == full.freeze.max()
    assert full.freeze[3] == 0 and not full.x[:, 3].any() and full.thr[3] == 0.0
    assert (full.freeze[:3] > 5).all()
    np.testing.assert_allclose(full.thr[:3], 1e-6 * np.linalg.norm(b.astype(np.float64), axis=0)[:3], rtol=1e-15)
    assert (full.true_rnorm <= full.thr).all() and (full.rnorm <= full.thr).all()
    for c in range(3):
        one = ss.pcg(A, b[:, c:c + 1], rtol=1e-6)
        assert one.freeze[0] == full.freeze[c] == one.iterations
        assert np.abs(one.x[:, 0] - full.x[:, c]).max() <= 1e-12 * np.abs(full.x[:, c]).max()
        assert abs(one.rnorm[0] - full.rnorm[c]) <= 1e-12 * full.thr[c]
        # the iterate of this column after exactly `freeze` steps of the full solve is the one returned: later steps did not touch it
        at = ss.pcg(A, b, rtol=1e-6, max_iter=int(full.freeze[c]))
        assert np.array_equal(at.x[:, c], full.x[:, c]) and at.rnorm[c] == full.rnorm[c]
        before = ss.pcg(A, b, rtol=1e-6, max_iter=int(full.freeze[c]) - 1)
        assert before.true_rnorm[c] > full.thr[c] and not before.converged[c] and before.freeze[c] == full.freeze[c] - 1
    if n == 20:
        # the counts the issue of this test file was written from: 83 (cotangent) and 87 (uniform) iterations
        assert full.iterations == {"cot": 83, "uniform": 87}[kind]


@pytest.mark.parametrize("kind", ["cot", "uniform"])
def test_the_statement_is_jacobi_pcg_with_bookkeeping(kind):
    A, (r, c, val) = _system(4, kind)
    b = _scaled_rhs(A.shape[0], seed=1)
    for kw in (dict(rtol=1e-6), dict(rtol=1e-3), dict(rtol=0.0, atol=1e-4), dict(rtol=1e-6, max_iter=7)):
        x, it = osv.jacobi_pcg(r, c, val, b, **kw)
        st = ss.pcg(A, b, **kw)
        assert st.iterations == it
        assert np.abs(st.x - x).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cap_returns_the_iterate_after_exactly_max_iter_steps(dtype):
    A, _ = _system(4, "cot")
    b = _scaled_rhs(A.shape[0], seed=2)[:, :1]
    full = ss.pcg(A, b, rtol=1e-6, dtype=dtype)
    n = full.iterations
    assert n > 8
    prev = None
    for m in (0, 1, n - 5, n - 1, n, n + 3):
        st = ss.pcg(A, b, rtol=1e-6, max_iter=m, dtype=dtype)
        assert st.iterations == min(m, n) and st.freeze[0] == min(m, n) and bool(st.converged[0]) == (m >= n)
        assert st.x.dtype == dtype
        if m == 0:
            assert not st.x.any() and st.rnorm[0] == st.bnorm[0]
        if prev is not None and m <= n:
            assert st.true_rnorm[0] != prev.true_rnorm[0] and np.abs(st.x - prev.x).max() > 0        # every step moves the iterate
        if m >= n:
            assert np.array_equal(st.x, full.x)
        prev = st
    # a warm start at the solution is converged before the first step and is returned as it is
    warm = ss.pcg(A, b, x0=full.x, rtol=1e-3, dtype=dtype)
    assert warm.iterations == 0 and np.array_equal(warm.x, full.x)


def test_frozen_and_running_columns_together():
    """The freeze case of the GPU tests: a smooth right-hand side M 1 next to a random one stops early and stays."""
    A, _ = _system(20, "uniform")
    V = A.shape[0]
    b = np.stack([np.random.default_rng(0).standard_normal(V), A @ np.ones(V)], 1).astype(np.float32)
    both = ss.pcg(A, b, rtol=1e-6)
    assert both.freeze[1] < both.freeze[0] - 20 and both.iterations == both.freeze[0]
    alone = ss.pcg(A, b[:, 1:], rtol=1e-6)
    assert alone.freeze[0] == both.freeze[1] and np.abs(alone.x[:, 0] - both.x[:, 1]).max() <= 1e-12
    assert np.abs(both.x[:, 1] - 1.0).max() <= 1e-5


def test_fp32_margins_of_the_issue():
    """What the fp32 recurrence reaches on the 4002-vertex sphere: within its threshold at rtol = 1e-3, up to ~2 x at rtol = 1e-6."""
    for kind in ("cot", "uniform"):
        A, _ = _system(20, kind)
        b = _scaled_rhs(A.shape[0])
        for rtol, lo, hi in ((1e-3, 0.5, 1.0), (1e-6, 1.0, 4.0)):
            st = ss.pcg(A, b, rtol=rtol, dtype=np.float32)
            ratio = st.true_rnorm[:3] / st.thr[:3]
            assert st.converged.all() and (st.rnorm <= st.thr).all()
            assert lo < ratio.max() <= hi, f"{kind} rtol={rtol}: {ratio}"
            assert abs(st.iterations - ss.pcg(A, b, rtol=rtol).iterations) <= 2


def test_chebyshev_count_at_a_hand_computed_point():
    """lmax / lmin = 9 after the safeguards -> sqrt = 3 -> rate = 1/2: n = ceil(log2(2 / target))."""
    lmin, lmax = 1.0 / 0.98, 9.0 / (1.0 + 1e-5)
    lo, hi, rate = ss.chebyshev_rate(lmin, lmax)
    assert abs(lo - 1.0) < 1e-15 and abs(hi - 9.0) < 1e-14 and abs(rate - 0.5) < 1e-15
    assert ss.chebyshev_count(lmin, lmax, rtol=1e-3) == 11           # log2(2000) = 10.97
    assert ss.chebyshev_count(lmin, lmax, rtol=1e-6) == 21           # log2(2e6) = 20.93
    assert ss.chebyshev_count(lmin, lmax, rtol=1.0) == 0
    # per-column form: the column furthest from its threshold decides; a column inside its threshold does not count
    assert ss.chebyshev_count(lmin, lmax, thr=[1e-3, 5.0], r0=[1.0, 1.0]) == 11
    assert ss.chebyshev_count(lmin, lmax, thr=[1e-3, 1e-3], r0=[1e-4, 1.0]) == 11
    assert ss.chebyshev_count(lmin, lmax, thr=[1e-3, 1e-3], r0=[1e-4, 1e-3]) == 0
    assert ss.chebyshev_count(lmin, lmax, thr=[1e-3, 1e-3], r0=[1000.0, 1.0]) == 21
    assert ss.chebyshev_count(lmin, lmax, thr=[0.0], r0=[1.0]) == math.ceil(math.log2(2e30))
    # a realistic enclosure (uniform Laplacian, lambda = 25, valence 6): the formula of ls_solver_chebyshev_iterations written out
    lmin, lmax = 1.0 / 151.0, 301.0 / 151.0
    sk = math.sqrt(lmax * (1 + 1e-5) / (0.98 * lmin))
    assert ss.chebyshev_count(lmin, lmax, rtol=1e-6) == math.ceil(math.log(2e6) / -math.log((sk - 1) / (sk + 1))) == 127
