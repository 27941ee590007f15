"""
The stopping contract of the iterative solvers (csrc/pcg.hip, largesteps/solvers.py), stated in plain numpy / scipy.

    pcg(...)               Jacobi-preconditioned CG with the rule of PCGSolver: column c is converged when ||r_c||_2 <= max(rtol ||b_c||_2,
                           atol); a converged column is FROZEN (its iterate, residual and reported norm stay what they were at that
                           iteration) while the others go on; max_iter bounds the work. It is oracle.solve.jacobi_pcg (which stays as it is:
                           others call it) with the per-column bookkeeping added.
    chebyshev_count(...)   the a-priori iteration count of the Chebyshev-Jacobi path as solve_cheb computes it from the enclosure that
                           ls_solver_spectrum reports.

dtype=np.float64 is the definition. dtype=np.float32 is what an fp32 run of the same recurrence can reach: vectors, the matrix product and the
scalars alpha, beta in fp32, the dot products accumulated in fp64 -- the number formats of the kernels, without their fused multiply-adds and
their summation order. The GPU tests take their margins from it (tests/test_stopping_gpu.py), never from the kernels' own output.
"""
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp


def system_matrix(rows, cols, vals, V):
    """the fp64 scipy matrix of the (fp32-assembled) COO entries"""
    return sp.csr_matrix((np.asarray(vals).astype(np.float64), (np.asarray(rows), np.asarray(cols))), shape=(V, V))


def thresholds(b, rtol, atol):
    """max(rtol ||b_c||_2, atol) per column, norms in fp64"""
    b64 = np.asarray(b).astype(np.float64)
    return np.maximum(rtol * np.linalg.norm(b64, axis=0), atol)


def true_residual(A, x, b):
    """||b_c - A x_c||_2 in fp64, per column"""
    return np.linalg.norm(np.asarray(b).astype(np.float64) - A @ np.asarray(x).astype(np.float64), axis=0)


def pcg(A, b, x0=None, rtol=1e-6, atol=0.0, max_iter=10000, dtype=np.float64):
    """
    A: scipy sparse (V, V), symmetric positive definite; b: (V, k); x0: (V, k) or None (zero).

    Returns a namespace with, per column,
        freeze      the iteration at which the column froze (0: the start already met the rule); max_iter for a column still active at the cap
        x           (V, k) in `dtype`: the iterate at the freeze (or after max_iter steps)
        rnorm       the norm of the RECURRENCE residual at that point (what the solver reports)
        true_rnorm  ||b - A x||_2 of that iterate, evaluated in fp64
        thr, bnorm  the threshold and ||b||_2 (fp64)
        converged   per column
    and `iterations`: the largest freeze iteration (max_iter if a column was still active at the cap).
    """
    A64 = sp.csr_matrix(A).astype(np.float64)
    M = A64.astype(dtype)
    b = np.asarray(b)
    if b.ndim != 2:
        raise ValueError("b must be (V, k)")
    b = b.astype(dtype)
    k = b.shape[1]
    dinv = (1.0 / M.diagonal()).astype(dtype)

    # Every column is multiplied and summed on its own contiguous copy, so that a column's arithmetic does not depend on how many columns
    # travel with it: a k-column solve is the k single-column solves, bit for bit.
    def dot(u, w):      # products of `dtype` numbers accumulated in fp64
        return np.array([np.sum(np.ascontiguousarray(u[:, c]).astype(np.float64) * np.ascontiguousarray(w[:, c]).astype(np.float64))
                         for c in range(k)])

    def matvec(u):
        return np.stack([M @ np.ascontiguousarray(u[:, c]) for c in range(k)], 1).astype(dtype)

    x = np.zeros_like(b) if x0 is None else np.asarray(x0).astype(dtype).copy()
    r = b if x0 is None else (b - matvec(x)).astype(dtype)
    r = r.copy()
    z = (dinv[:, None] * r).astype(dtype)
    p = z.copy()
    rz = dot(r, z)
    rr = dot(r, r)
    thr = thresholds(b, rtol, atol)
    active = rr > thr * thr
    freeze = np.where(active, -1, 0)
    it = 0
    while active.any() and it < max_iter:
        Ap = matvec(p)
        pAp = dot(p, Ap)
        ok = active & (pAp > 0)
        alpha = np.where(ok, rz / np.where(ok, pAp, 1.0), 0.0).astype(dtype)
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * Ap).astype(dtype)
        z = (dinv[:, None] * r).astype(dtype)
        rz_new = dot(r, z)
        beta = np.where(active & (rz > 0), rz_new / np.where(rz > 0, rz, 1.0), 0.0).astype(dtype)
        p = (z + beta * p).astype(dtype)
        rz = np.where(active, rz_new, rz)
        rr = np.where(active, dot(r, r), rr)
        it += 1
        still = active & (rr > thr * thr)
        freeze = np.where(active & ~still, it, freeze)
        active = still
    freeze = np.where(active, max_iter, freeze)
    return SimpleNamespace(freeze=freeze.astype(int), x=x, rnorm=np.sqrt(rr), true_rnorm=true_residual(A64, x, b), thr=thr,
                           bnorm=np.linalg.norm(b.astype(np.float64), axis=0), converged=~active,
                           iterations=int(max_iter if active.any() else freeze.max(initial=0)))


def chebyshev_rate(lmin, lmax):
    """(lmin, lmax) as ls_solver_spectrum returns them -> the safeguarded enclosure solve_cheb iterates on and its convergence rate"""
    lo, hi = 0.98 * lmin, lmax * (1.0 + 1e-5)
    sk = math.sqrt(hi / lo)
    return lo, hi, (sk - 1.0) / (sk + 1.0)


def chebyshev_count(lmin, lmax, rtol=None, thr=None, r0=None):
    """
    The Chebyshev iteration count: n = ceil(log(2 / target) / -log(rate)), 0 when nothing is left to do.

    Cold start without atol: chebyshev_count(lmin, lmax, rtol=rtol)  (||r0|| = ||b||: target = rtol).
    Otherwise: thr, r0 = per-column threshold and starting residual norm; target = the smallest thr / r0 over the columns that do not meet
    their threshold yet (a threshold of 0 asks for 1e-30).
    """
    _, _, rate = chebyshev_rate(lmin, lmax)
    if thr is None:
        target = float(rtol)
    else:
        target = 1.0
        for t, r in zip(np.atleast_1d(thr), np.atleast_1d(r0)):
            if r > t:
                target = min(target, t / r)
    if target >= 1.0:
        return 0
    return int(math.ceil(math.log(2.0 / max(target, 1e-30)) / -math.log(rate)))
