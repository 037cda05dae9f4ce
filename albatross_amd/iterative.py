"""The matrix-free exact fit (agp_gram_matvec, agp_iterative_*).

    out = ab.gram_matvec(cov, x, V, targets_variance=None)        # (cov(x, x) + diag(targets_variance)) @ V
    fm = model.fit_iterative(dataset, preconditioner_rank=256, tolerance=1e-10)
    fm.predict(xs).mean(); fm.predict(xs).marginal(); fm.get_fit().information / .iterations / .residual / .solve(rhs)

K = cov(x, x) is evaluated pair by pair inside the product on the device and never stored: memory is O(n * columns)
instead of O(n^2).  Every entry has the bits `Context.gram(cov, x)` gives it.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from .covariance import Measurement, has_linear_combinations
from .gp import AlbatrossAmdError, DeviceArray, MarginalDistribution, _ptr, _values_of, default_context

MATVEC_MAX_RHS = 16  # AGP_MATVEC_MAX_RHS: right-hand sides that share one evaluation of an entry


def gram_matvec(cov, features, V, targets_variance=None, on_device=False, context=None):
    """(cov(features) + diag(targets_variance)) @ V for V of shape (n,) or (n, columns).  `features` may be a
    `_capi.Features` record whose arrays already live on the device; `on_device=True` takes V as a DeviceArray of shape
    (n, columns) - its bytes column-major - and returns one (targets_variance then is a DeviceArray or None when
    `features` lives there too, a numpy array otherwise)."""
    ctx = context or default_context()
    if isinstance(features, capi.Features):
        keep, s = None, features
    else:
        if has_linear_combinations(features):
            raise ValueError("gram_matvec: LinearCombination features are not supported")
        keep = cov.features(features)
        s = keep.as_struct()
    n = int(s.n)
    if n == 0:
        raise ValueError("gram_matvec: no features")
    if targets_variance is None:
        vp = None
    elif isinstance(targets_variance, DeviceArray):
        if s.location != capi.DEVICE:
            raise ValueError("gram_matvec: targets_variance lives where the features live")
        vp = C.c_void_p(targets_variance.ptr)
    else:
        if s.location != capi.HOST:
            raise ValueError("gram_matvec: targets_variance lives where the features live")
        var = np.ascontiguousarray(targets_variance, dtype=np.float64)
        if var.shape != (n,):
            raise ValueError("gram_matvec: targets_variance must have one value per feature")
        vp = _ptr(var)
    if on_device:
        if not isinstance(V, DeviceArray) or len(V.shape) != 2 or V.shape[0] != n:
            raise ValueError("gram_matvec: on_device=True takes a DeviceArray of shape (n, columns)")
        cols = int(V.shape[1])
        out = ctx.device_empty((n, cols))
        st = ctx._lib.agp_gram_matvec(ctx._h, ctx.kernel(cov), C.byref(s), vp, C.c_void_p(V.ptr), n, cols, C.c_void_p(out.ptr), n,
                                      capi.DEVICE)
        ctx._check(st, "agp_gram_matvec")
        return out
    Vh = np.asarray(V, dtype=np.float64)
    one = Vh.ndim == 1
    Vh = np.asfortranarray(Vh.reshape(n, -1) if Vh.shape[0] == n else Vh)
    if Vh.ndim != 2 or Vh.shape[0] != n or Vh.shape[1] < 1:
        raise ValueError("gram_matvec: V must have one row per feature and at least one column")
    out = np.empty(Vh.shape, order="F")
    st = ctx._lib.agp_gram_matvec(ctx._h, ctx.kernel(cov), C.byref(s), vp, _ptr(Vh), n, Vh.shape[1], _ptr(out), n, capi.HOST)
    ctx._check(st, "agp_gram_matvec")
    return out[:, 0].copy() if one else out


class NotConvergedError(AlbatrossAmdError):
    """AGP_ERR_NOT_CONVERGED: max_iterations reached with a right-hand side still above the tolerance; carries the
    `iterations` carried out and the final relative `residual` of the recurrence."""

    def __init__(self, status, detail="", iterations=None, residual=None):
        super().__init__(status, detail)
        self.iterations = iterations
        self.residual = residual


def _raise(ctx, st, what, iterations=None, residual=None):
    if st == capi.AGP_ERR_NOT_CONVERGED:
        raise NotConvergedError(st, what, iterations, residual)
    ctx._check(st, what)


class IterativeGPFit:
    """agp_iterative_fit: the matrix-free fit.  `information` = (K + diag(var))^-1 (y - mean), `iterations` and
    `residual` of the conjugate-gradient solve that produced it, `preconditioner_rank` of the pivoted Cholesky factor
    that preconditions it (below the requested rank when the points ran out: duplicates), `solve(rhs)`."""

    def __init__(self, ctx, handle, n, train_features, information, iterations, residual):
        self._ctx, self._h, self.n = ctx, handle, n
        self.train_features = train_features
        self.information = information
        self.iterations = iterations
        self.residual = residual
        self.preconditioner_rank = int(ctx._lib.agp_iterative_fit_preconditioner_rank(handle))

    def solve(self, rhs, return_info=False):
        """(K + diag(var))^-1 rhs for rhs of shape (n,) or (n, columns), at the fit's tolerance; return_info=True also
        returns the per-column iterations and residuals"""
        B = np.asarray(rhs, dtype=np.float64)
        one = B.ndim == 1
        B = np.asfortranarray(B.reshape(self.n, -1))
        cols = B.shape[1]
        out = np.empty((self.n, cols), order="F")
        its = np.zeros(cols, dtype=np.int32)
        res = np.zeros(cols)
        st = self._ctx._lib.agp_iterative_solve(self._ctx._h, self._h, _ptr(B), self.n, cols, _ptr(out), self.n, capi.HOST,
                                                _ptr(its), _ptr(res))
        _raise(self._ctx, st, "agp_iterative_solve", its, res)
        x = out[:, 0].copy() if one else out
        return (x, its, res) if return_info else x

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._lib.agp_iterative_fit_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IterativePrediction:
    """`.mean()` and `.marginal()` of a matrix-free fit; `.joint()` is out of scope (it needs the m x m posterior
    covariance, i.e. m solves against a matrix that is never formed - use the dense fit)."""

    def __init__(self, fit_model, features):
        self._fm, self._features = fit_model, features

    def mean(self):
        return self._fm._predict(self._features, False)

    def marginal(self):
        return self._fm._predict(self._features, True)

    def joint(self, on_device=False):
        raise NotImplementedError("fit_iterative: joint predictions are not supported by the matrix-free fit; "
                                  "use .marginal(), or model.fit(dataset) for a joint distribution")


class IterativeFitModel:
    """What `GaussianProcessRegression.fit_iterative` returns."""

    def __init__(self, model, fit):
        self._model, self._fit = model, fit

    def get_fit(self):
        return self._fit

    def get_model(self):
        return self._model

    def predict(self, features):
        return IterativePrediction(self, features)

    def predict_with_measurement_noise(self, features):
        return IterativePrediction(self, features if isinstance(features, Measurement) else Measurement(features))

    def _predict(self, features, marginal):
        m, ctx = self._model, self._fit._ctx
        if has_linear_combinations(features):
            raise ValueError("fit_iterative: LinearCombination features are not supported")
        fs = m.covariance_function_.features(features)
        s = fs.as_struct()
        mean = np.empty(fs.n)
        kh = ctx.kernel(m.covariance_function_)
        if not marginal:
            ctx._check(ctx._lib.agp_iterative_predict_mean(ctx._h, kh, self._fit._h, C.byref(s), _ptr(mean), capi.HOST),
                       "agp_iterative_predict_mean")
            return mean + m.mean_function_(fs.coords)
        var = np.empty(fs.n)
        st = ctx._lib.agp_iterative_predict_marginal(ctx._h, kh, self._fit._h, C.byref(s), _ptr(mean), _ptr(var), capi.HOST)
        _raise(ctx, st, "agp_iterative_predict_marginal")
        return MarginalDistribution(mean + m.mean_function_(fs.coords), var)


def fit_iterative(model, dataset, preconditioner_rank=256, preconditioner_tolerance=1e-12, tolerance=1e-10, max_iterations=1000):
    """`GaussianProcessRegression.fit_iterative`: the exact fit without the n x n covariance - preconditioned conjugate
    gradients around `gram_matvec`, preconditioned by the rank-`preconditioner_rank` pivoted Cholesky factor (0: plain
    CG).  The mean function is removed from the targets exactly as `fit` does.  Raises NotConvergedError when
    `max_iterations` do not reach `tolerance` (relative residual)."""
    ctx = model._ctx()
    if has_linear_combinations(dataset.features):
        raise ValueError("fit_iterative: LinearCombination features are not supported")
    fs = model.covariance_function_.features(_values_of(dataset.features))
    y, yv = model._targets(fs, dataset.targets)
    s = fs.as_struct()
    opt = capi.IterativeOptions(int(preconditioner_rank), float(preconditioner_tolerance), float(tolerance), int(max_iterations))
    h = C.c_void_p()
    info = np.empty(fs.n)
    it, res = C.c_int(0), C.c_double(0.)
    st = ctx._lib.agp_iterative_fit_create(ctx._h, ctx.kernel(model.covariance_function_), C.byref(s), _ptr(y), _ptr(yv),
                                           C.byref(opt), C.byref(h), _ptr(info), C.byref(it), C.byref(res))
    _raise(ctx, st, "agp_iterative_fit_create", it.value, res.value)
    return IterativeFitModel(model, IterativeGPFit(ctx, h, fs.n, dataset.features, info, it.value, res.value))
