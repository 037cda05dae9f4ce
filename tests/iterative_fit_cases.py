"""Shared by tests/test_iterative_fit_host.py and tests/test_iterative_fit_gpu.py: the inputs, the bounds and a float64 numpy
restatement of the matrix-free fit (csrc/iterative.hip; include/albatross_amd.h, "matrix-free fit").

The definition restated here:
    A = K + diag(y_var);  (L, m, trace) = the greedy pivoted Cholesky of A (tests/pivoted_chol_cases.py: restatement) with
    max_rank = min(precond_rank, n);  delta = max(trace / (n - m), 1e-8 max_i A_ii), the floor alone when m = n;
    P^-1 r = (r - L (delta I + L^T L)^-1 L^T r) / delta;  rank 0: delta = mean(diag A), P = delta I.
    Preconditioned conjugate gradients from x = 0; a column stops at the first iteration k with ||r_k|| <= tol ||b||;
    A_ii <= 0: not positive definite before any iteration; p^T A p <= 0: not positive definite; a zero b: x = 0, 0 iterations.

Bounds (nothing measured):
  * information against the dense fit: max|a - a_dense| <= 1e-8 max|a_dense|, the project's parity bar.
  * the true relative residual ||y - A a|| / ||y||, recomputed in longdouble from ctx.gram's matrix, is at most
        tolerance + gamma(L + S + 2) || |A| |a| || / ||y||
    the recurrence's residual meets the tolerance by the stop rule, and what separates it from the true residual is the
    rounding of the products it was updated with; the floor charged here is that of ONE product A a in the kernel's
    summation structure (tests/gram_matvec_cases.py: gamma(L + S)), plus two roundings for the update of r.
"""
import functools

import numpy as np

import albatross_amd as ab

import gram_matvec_cases as mc
import pivoted_chol_cases as pc

TOL = 1e-10
PARITY = 1e-8
DELTA_FLOOR = 1e-8


def _se_noise(length=1., sigma_noise=0.1):
    return ab.SquaredExponential(length, 1.) + ab.IndependentNoise(sigma_noise)


def _uniform(n, dim, hi, seed):
    return np.random.default_rng(seed).uniform(0., hi, (n, dim))


def _duplicates():
    """40 distinct 2-D points, each present five times: the pivoted Cholesky of the noise-free tree stops at rank 40"""
    base = _uniform(40, 2, 6., 77)
    return np.tile(base, (5, 1))


# name: (n, points, covariance builder)
CASES = {
    "n1": (1, lambda: _uniform(1, 3, 4., 1), _se_noise),
    "n2": (2, lambda: _uniform(2, 3, 4., 2), _se_noise),
    "n65_3d": (65, lambda: _uniform(65, 3, 4., 3), _se_noise),
    "n777_2d": (777, lambda: _uniform(777, 2, 10., 4), functools.partial(_se_noise, 1.5, 0.05)),
    "n1500_1d": (1500, lambda: _uniform(1500, 1, 30., 5), _se_noise),
}
ONE_D = "n1500_1d"
RANKS = [0, 1, 64, "n"]
# duplicated points, no noise term in the tree, y_var given (without it the matrix is singular): once every distinct point
# is chosen, the residual diagonal of a copy is the sum of two variances, <= 0.4 < DUPLICATE_REL_TOL max_i A_ii - the
# pivoted Cholesky stops below the rank asked for
DUPLICATES = (200, _duplicates, lambda: ab.SquaredExponential(1., 1.))
DUPLICATE_RANK_ASKED, DUPLICATE_DISTINCT, DUPLICATE_REL_TOL = 64, 40, 0.5


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(cov, x, y, y_var): never modified"""
    n, make, cov = DUPLICATES if name == "duplicates" else CASES[name]
    x = make()
    rng = np.random.default_rng(1000 + n)
    y = np.sin(x).sum(axis=1) + 0.1 * rng.standard_normal(n)
    y_var = rng.uniform(0.02, 0.2, n)
    for a in (x, y, y_var):
        a.setflags(write=False)
    return cov(), x, y, y_var


def rank_of(r, n):
    return n if r == "n" else min(r, n)


def query_points(m, dim, hi, seed=9):
    return _uniform(m, dim, hi, seed)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
class Preconditioner:
    def __init__(self, A, precond_rank, rel_tol=1e-12):
        n = A.shape[0]
        d = np.diag(A).copy()
        self.n, self.d0 = n, d.max()
        want = min(precond_rank, n)
        if want > 0:
            _, self.rank, self.L, _, trace = pc.restatement(d, lambda p: A[:, p], want, rel_tol)
            trace = float(trace)
        else:
            self.rank, self.L, trace = 0, np.zeros((n, 0)), float(d.sum())
        floor = DELTA_FLOOR * self.d0
        self.delta = max(trace / (n - self.rank), floor) if self.rank < n else floor
        if self.rank:
            self.chol = np.linalg.cholesky(self.delta * np.eye(self.rank) + self.L.T @ self.L)

    def apply(self, r):
        if not self.rank:
            return r / self.delta
        t = self.L.T @ r
        u = np.linalg.solve(self.chol.T, np.linalg.solve(self.chol, t))
        return (r - self.L @ u) / self.delta


OK, NOT_CONVERGED, NOT_POSITIVE_DEFINITE, NAN_INPUT = "ok", "not converged", "not positive definite", "nan"


def pcg(A, b, precond_rank, tol=TOL, max_iterations=1000, rel_tol=1e-12):
    """(status, x, iterations, relative residual of the recurrence, preconditioner rank) for ONE right-hand side"""
    n = A.shape[0]
    if np.isnan(A).any() or np.isnan(b).any():
        return NAN_INPUT, None, 0, 0., 0
    if np.diag(A).min() <= 0.:
        return NOT_POSITIVE_DEFINITE, None, 0, 0., 0
    P = Preconditioner(A, precond_rank, rel_tol)
    x = np.zeros(n)
    bb = float(b @ b)
    if bb == 0.:
        return OK, x, 0, 0., P.rank
    r = b.copy()
    p = None
    rz_old = 0.
    resid = 1.
    for k in range(max_iterations):
        z = P.apply(r)
        rz = float(r @ z)
        p = z if k == 0 else z + (rz / rz_old) * p
        q = A @ p
        pq = float(p @ q)
        if pq <= 0.:
            return NOT_POSITIVE_DEFINITE, None, k, resid, P.rank
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        rz_old = rz
        resid = np.sqrt(float(r @ r)) / np.sqrt(bb)
        if np.sqrt(float(r @ r)) <= tol * np.sqrt(bb):
            return OK, x, k + 1, resid, P.rank
    return NOT_CONVERGED, x, max_iterations, resid, P.rank


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def system(K, y_var):
    return mc.system_matrix(K, y_var)


def residual_bound(A, a, y, tol=TOL):
    n = A.shape[0]
    S, cps = mc.slices(n)
    floor = mc.gamma(min(cps, n) + S + 2) * np.linalg.norm(np.abs(A) @ np.abs(a)) / np.linalg.norm(y)
    return tol + floor


def true_residual(A, a, y):
    LD = np.longdouble
    r = y.astype(LD) - A.astype(LD) @ np.asarray(a, dtype=np.float64).astype(LD)
    return float(np.sqrt((r * r).sum()) / np.sqrt((y.astype(LD) ** 2).sum()))


def check_information(A, a, a_dense, y, tol=TOL):
    """asserts the two bounds; returns (parity error / bar, true residual / bound)"""
    err = np.abs(a - a_dense).max() / np.abs(a_dense).max()
    res, bound = true_residual(A, a, y), residual_bound(A, a, y, tol)
    assert err <= PARITY, ("information against the dense solve", err)
    assert res <= bound, ("true relative residual", res, bound)
    return err / PARITY, res / bound
