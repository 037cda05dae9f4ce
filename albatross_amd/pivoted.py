"""Greedy pivoted Cholesky factorisation of a covariance (agp_pivoted_cholesky) and the inducing-point strategy
built on it.

    f = ab.pivoted_cholesky(cov, x, 256, tolerance=1e-10)
    f.pivots, f.rank, f.factor, f.residual_diagonal, f.trace_residual      # K ~ factor factor^T
    model = ab.sparse_gp_from_covariance(cov, grouper, ab.GreedyVarianceInducingPoints(256))

The factorisation runs on the device, column by column, without ever storing K = cov(x, x).
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from .covariance import Measurement, has_linear_combinations
from .gp import _ptr, default_context


class PivotedCholesky:
    """What `pivoted_cholesky` returns: `pivots` (rank indices, in the order they were chosen), `rank`, `factor`
    (n x rank: a numpy array, a DeviceArray of shape (n, max_rank) whose first `rank` columns are written - its bytes
    are column-major - or None), `residual_diagonal` (n values: diag(K - L L^T), exactly 0 at the pivots) and
    `trace_residual` (their sum)."""

    def __init__(self, pivots, rank, factor, residual_diagonal, trace_residual):
        self.pivots = pivots
        self.rank = rank
        self.factor = factor
        self.residual_diagonal = residual_diagonal
        self.trace_residual = trace_residual


def pivoted_cholesky(cov, features, max_rank, tolerance=0.0, want_factor=True, on_device=False, context=None):
    """The partial Cholesky factorisation of K = cov(features) with diagonal pivoting (greedy conditional-variance
    selection): step j picks the unselected point with the largest residual variance d (the lowest index on equal
    values) and stops when that is <= tolerance * max_i K_ii or <= 0, else appends the column
    L[:, j] = (K[:, p] - L[:, :j] L[p, :j]) / sqrt(d_p) and lowers d by its squares.  `max_rank` is clipped to n.
    `on_device=True` leaves factor and residual_diagonal in HBM (DeviceArrays); `features` may be a `_capi.Features`
    record whose arrays already live there."""
    ctx = context or default_context()
    if isinstance(features, capi.Features):
        fs, s = None, features
    else:
        if has_linear_combinations(features):
            raise ValueError("pivoted_cholesky: LinearCombination features are not supported")
        fs = cov.features(features)
        s = fs.as_struct()
    n = int(s.n)
    if n == 0:
        raise ValueError("pivoted_cholesky: no features")
    m = min(int(max_rank), n)
    pivots = np.empty(max(m, 1), dtype=np.int64)
    rank = C.c_int64(0)
    trace = C.c_double(0.)
    location = capi.DEVICE if on_device else capi.HOST
    if on_device:
        factor = ctx.device_empty((n, m)) if want_factor else None
        resid = ctx.device_empty((n,))
        lp, rp = (C.c_void_p(factor.ptr) if want_factor else None), C.c_void_p(resid.ptr)
    else:
        factor = np.empty((n, m), order="F") if want_factor else None
        resid = np.empty(n)
        lp, rp = _ptr(factor), _ptr(resid)
    ctx._check(ctx._lib.agp_pivoted_cholesky(ctx._h, ctx.kernel(cov), C.byref(s), m, float(tolerance), _ptr(pivots),
                                             C.byref(rank), lp, n, rp, location, C.byref(trace)), "agp_pivoted_cholesky")
    r = int(rank.value)
    if factor is not None and not on_device:
        factor = factor[:, :r]
    return PivotedCholesky(pivots[:r].copy(), r, factor, resid, float(trace.value))


class GreedyVarianceInducingPoints:
    """An InducingPointStrategy: the `num_points` features that the greedy pivoted Cholesky factorisation of
    cov(features) selects, in the order it selects them - each one the point whose prior variance is least explained by
    those already chosen.  Fewer are returned when the largest residual variance falls to `tolerance` times the largest
    prior variance first (duplicates of a chosen point are never chosen: their residual is rounding dust, which a
    tolerance of 0 would go on to select); `num_points` is clipped to the number of features.

    The selection sees the covariance of the plain features: `measurement_only` terms are zero for it, as they are in
    K_uu.  An unwrapped IndependentNoise term raises every diagonal entry, so the selection sees it and the residual
    never falls below it.  LinearCombination features raise ValueError."""

    def __init__(self, num_points, tolerance=1e-12, context=None):
        self.num_points = int(num_points)
        self.tolerance = float(tolerance)
        self._context = context

    def __call__(self, cov, features):
        if has_linear_combinations(features):
            raise ValueError("GreedyVarianceInducingPoints: LinearCombination features are not supported")
        values = features.values if isinstance(features, Measurement) else features
        f = pivoted_cholesky(cov, values, self.num_points, self.tolerance, want_factor=False, context=self._context)
        return np.asarray(values, dtype=np.float64)[f.pivots]
