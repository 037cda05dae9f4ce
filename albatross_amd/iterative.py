"""The matrix-free exact fit (agp_gram_matvec, agp_iterative_*).

    out = ab.gram_matvec(cov, x, V, targets_variance=None)        # (cov(x, x) + diag(targets_variance)) @ V
    fm = model.fit_iterative(dataset, preconditioner_rank=256, tolerance=1e-10)
    fm.predict(xs).mean(); fm.predict(xs).marginal(); fm.get_fit().information / .iterations / .residual / .solve(rhs)
    forms = ab.gram_tangent_forms(cov, x, U, V)                   # {name: U[:, c] @ d cov(x, x) / d name @ V[:, c]}
    grad, stderr = fm.log_likelihood_gradient(num_probes=16, seed=0)   # probe estimate, no log-determinant
    value, stderr = fm.log_likelihood(num_probes=16, seed=0)           # stochastic Lanczos quadrature
    value, stderr, grad, grad_stderr = fm.log_likelihood_and_gradient(num_probes=16, seed=0)   # one chain of solves

K = cov(x, x) is evaluated pair by pair inside the product on the device and never stored: memory is O(n * columns)
instead of O(n^2).  Every entry has the bits `Context.gram(cov, x)` gives it.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from .covariance import Measurement, has_linear_combinations
from .gp import AlbatrossAmdError, DeviceArray, MarginalDistribution, _ptr, _values_of, default_context

MATVEC_MAX_RHS = 16  # AGP_MATVEC_MAX_RHS: right-hand sides that share one evaluation of an entry
TANGENT_FORMS_MAX_PAIRS = 8  # AGP_TANGENT_FORMS_MAX_PAIRS: column pairs that share one evaluation of a pair's tangents


def _slot_tables(cov, fs):
    """(slots, ctypes table, tangent columns or None) of `cov` at the features, as gp._gradient_problem builds them"""
    slots, columns = cov.param_slots()
    if len(slots) > capi.MAX_GRADIENT_SLOTS:
        raise ValueError(f"more than {capi.MAX_GRADIENT_SLOTS} covariance parameter slots")
    tangents = None
    if columns:
        tangents = np.empty((fs.n, len(columns)), order="F")
        for c, (fn, name) in enumerate(columns):
            tangents[:, c] = fn.derivative(fs.coords, name)
    table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(node, p) for node, p, _ in slots])
    return slots, table, tangents


def gram_tangent_forms(cov, features, U, V, names=None, on_device=False, context=None):
    """{name: array[ncols]} with entry c = U[:, c] @ (d cov(features, features) / d name) @ V[:, c] for every parameter
    name of `cov` (or those in `names`), the derivative matrix evaluated pair by pair on the device and never stored
    (agp_gram_tangent_forms).  Slots that share a name are summed.  U, V: shape (n,) or (n, ncols); `on_device=True`
    takes both as DeviceArrays of shape (n, ncols).  The features are taken as given: wrap them in Measurement for the
    matrix a fit factors."""
    ctx = context or default_context()
    if has_linear_combinations(features):
        raise ValueError("gram_tangent_forms: LinearCombination features are not supported")
    fs = cov.features(features)
    n = fs.n
    if n == 0:
        raise ValueError("gram_tangent_forms: no features")
    slots, table, tangents = _slot_tables(cov, fs)
    if names is not None:
        unknown = set(names) - {name for _, _, name in slots}
        if unknown:
            raise KeyError(f"gram_tangent_forms: no covariance parameter named {sorted(unknown)}")
    s = fs.as_struct()
    keep = []
    if on_device:
        for M in (U, V):
            if not isinstance(M, DeviceArray) or len(M.shape) != 2 or M.shape[0] != n:
                raise ValueError("gram_tangent_forms: on_device=True takes DeviceArrays of shape (n, columns)")
        if U.shape != V.shape:
            raise ValueError("gram_tangent_forms: U and V must have the same shape")
        ncols = int(U.shape[1])
        up, vp, loc = C.c_void_p(U.ptr), C.c_void_p(V.ptr), capi.DEVICE
        tp = None
        if tangents is not None:
            td = ctx.to_device(np.ascontiguousarray(tangents.T))  # (the bytes of the column-major n x columns matrix)
            keep.append(td)
            tp = C.c_void_p(td.ptr)
    else:
        Uh, Vh = (np.asfortranarray(np.asarray(M, dtype=np.float64).reshape(n, -1)) for M in (U, V))
        if Uh.shape != Vh.shape:
            raise ValueError("gram_tangent_forms: U and V must have the same shape")
        ncols = Uh.shape[1]
        up, vp, loc, tp = _ptr(Uh), _ptr(Vh), capi.HOST, _ptr(tangents)
    forms = np.zeros((max(1, ncols), max(1, len(slots))), order="F")
    st = ctx._lib.agp_gram_tangent_forms(ctx._h, ctx.kernel(cov), C.byref(s), len(slots), table, tp, n, up, n, vp, n, ncols,
                                         _ptr(forms), forms.shape[0], loc)
    ctx._check(st, "agp_gram_tangent_forms")
    out = {}
    for p, (_, _, name) in enumerate(slots):
        if names is None or name in names:
            out[name] = out.get(name, 0.) + forms[:ncols, p]
    return out


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

    def __init__(self, ctx, handle, n, train_features, information, iterations, residual, feature_set=None):
        self._ctx, self._h, self.n = ctx, handle, n
        self.train_features = train_features
        self.feature_set = feature_set  # the flattened features of the fit (the gradient's tangents are taken there)
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

    def _nll(self, num_probes, seed, probes, quadrature_tolerance, slots=(), table=None, tangents=None):
        """one agp_iterative_nll call: dict(nll, nll_stderr, log_det, samples (t), grad, grad_stderr (P each), grad_samples
        (t x P), iterations, residual)"""
        ctx, n = self._ctx, self.n
        if probes is None:
            t, pp, ldp = int(num_probes), None, 0
        else:
            Z = np.asfortranarray(np.asarray(probes, dtype=np.float64).reshape(n, -1))
            t, pp, ldp = Z.shape[1], _ptr(Z), n
        if t < 1:
            raise ValueError("log_likelihood: at least one probe")
        P = len(slots)
        nll, se, ld = C.c_double(), C.c_double(), C.c_double()
        samples = np.zeros(t)
        g, gse = np.zeros(max(1, P)), np.zeros(max(1, P))
        gs = np.zeros((t, max(1, P)), order="F")
        its, res = np.zeros(t, dtype=np.int32), np.zeros(t)
        qt = 0. if quadrature_tolerance is None else float(quadrature_tolerance)
        st = ctx._lib.agp_iterative_nll(ctx._h, self._h, t, int(seed), pp, ldp, capi.HOST, qt, P, table, _ptr(tangents), n,
                                        C.byref(nll), C.byref(se), C.byref(ld), _ptr(samples), _ptr(g), _ptr(gse), _ptr(gs), t,
                                        _ptr(its), _ptr(res))
        _raise(ctx, st, "agp_iterative_nll", its, res)
        return dict(nll=nll.value, nll_stderr=se.value, log_det=ld.value, samples=samples, grad=g[:P], grad_stderr=gse[:P],
                    grad_samples=gs[:, :P], iterations=its, residual=res)

    def log_determinant(self, num_probes=16, seed=0, probes=None, quadrature_tolerance=None, return_samples=False):
        """(log det(K + diag(var)), its standard error) by stochastic Lanczos quadrature (agp_iterative_nll): the closed-form
        log-determinant of the preconditioner plus the probe estimate of tr log of the preconditioned matrix - see
        `IterativeFitModel.log_likelihood` for the arguments.  return_samples=True: also the t per-probe samples."""
        r = self._nll(num_probes, seed, probes, quadrature_tolerance)
        out = (r["log_det"], 2. * r["nll_stderr"])
        return out + (r["samples"],) if return_samples else out

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
    """What `GaussianProcessRegression.fit_iterative` returns.  `gradient_iterations` / `gradient_residual`: per probe, the
    iterations and final relative residuals of the solves of the last `log_likelihood_gradient` call (None before one);
    `value_iterations` / `value_residual`: the same of the last `log_likelihood` / `log_likelihood_and_gradient` call."""

    gradient_iterations = None
    gradient_residual = None
    value_iterations = None
    value_residual = None

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

    def log_likelihood_gradient(self, num_probes=16, seed=0, probes=None, return_samples=False):
        """(grad, stderr): {name: d log p / d name} over every name of get_params() - the sign of
        `GaussianProcessRegression.log_likelihood_gradient` - and the standard error of each, WITHOUT the log-likelihood
        itself (agp_iterative_nll_gradient).  The trace term is estimated from `num_probes` Rademacher probes, a documented
        function of `seed`, or from the columns of `probes` (n x t, used as is; sqrt(n) * identity gives the exact
        gradient, stderr then measures nothing).  Slots that share a name have their samples summed before the standard
        error is taken.  Mean-function parameters are exact, (d mu / d name)^T alpha, with stderr 0.
        return_samples=True: also {name: array[t]} of the per-probe trace samples.  Raises NotConvergedError (with
        `iterations` and `residual` per probe) when a probe solve runs out of iterations.  After a call that returned,
        `gradient_iterations` and `gradient_residual` of this object hold the t probe solves' iteration counts and final
        relative residuals."""
        m, fit = self._model, self._fit
        ctx, fs, n = fit._ctx, fit.feature_set, fit.n
        cov = m.covariance_function_
        slots, table, tangents = _slot_tables(cov, fs)
        if probes is None:
            t, pp, ldp = int(num_probes), None, 0
        else:
            Z = np.asfortranarray(np.asarray(probes, dtype=np.float64).reshape(n, -1))
            t, pp, ldp = Z.shape[1], _ptr(Z), n
        if t < 1:
            raise ValueError("log_likelihood_gradient: at least one probe")
        P = len(slots)
        g, se = np.zeros(max(1, P)), np.zeros(max(1, P))
        samples = np.zeros((t, max(1, P)), order="F")
        its, res = np.zeros(t, dtype=np.int32), np.zeros(t)
        st = ctx._lib.agp_iterative_nll_gradient(ctx._h, fit._h, P, table, _ptr(tangents), n, t, int(seed), pp, ldp, capi.HOST,
                                                 _ptr(g), _ptr(se), _ptr(samples), t, _ptr(its), _ptr(res))
        _raise(ctx, st, "agp_iterative_nll_gradient", its, res)
        self.gradient_iterations, self.gradient_residual = its, res
        grad, stderr, by_name = self._gradient_by_name(slots, g, se, samples)
        if return_samples:
            return grad, stderr, by_name
        return grad, stderr

    def log_likelihood(self, num_probes=16, seed=0, probes=None, quadrature_tolerance=None, return_samples=False):
        """(value, stderr): the log-likelihood of the fitted dataset - the sign and the constant of
        `GaussianProcessRegression.log_likelihood` - and its standard error, by stochastic Lanczos quadrature
        (agp_iterative_nll).  log det A = log det P + tr log(P^-1/2 A P^-1/2): the first term in closed form from the
        preconditioner the fit holds, the trace estimated from `num_probes` probes z ~ N(0, P), a documented function of
        `seed`, whose conjugate-gradient coefficients are the Lanczos tridiagonal of the preconditioned matrix.  The data
        term is exact to the fit's tolerance.  The better the preconditioner, the smaller the standard error.
        probes: an n x t matrix used as z as is (sqrt(t) [L | sqrt(delta) I] with t = n + rank is exact).
        quadrature_tolerance: the relative residual at which a probe's recurrence stops; None: the fit's tolerance.
        return_samples=True: also the t per-probe samples of tr log.  Raises NotConvergedError like
        `log_likelihood_gradient`; `value_iterations` / `value_residual` hold the probe solves' counts after a call."""
        r = self._fit._nll(num_probes, seed, probes, quadrature_tolerance)
        self.value_iterations, self.value_residual = r["iterations"], r["residual"]
        out = (-r["nll"], r["nll_stderr"])
        return out + (r["samples"],) if return_samples else out

    def log_likelihood_and_gradient(self, num_probes=16, seed=0, probes=None, return_samples=False):
        """(value, stderr, grad, grad_stderr): `log_likelihood` and {name: d log p / d name} with its standard errors from
        ONE chain of probe solves (agp_iterative_nll): with w = A^-1 z and v = P^-1 z, E[w^T dA v] = tr(A^-1 dA) for
        z ~ N(0, P).  The solves run at the fit's tolerance.  Names, signs, shared names and mean-function parameters
        as in `log_likelihood_gradient` (whose Rademacher probes give other samples of the same trace).
        return_samples=True: also (the t samples of tr log, {name: array[t]} of the trace samples)."""
        m, fit = self._model, self._fit
        fs = fit.feature_set
        slots, table, tangents = _slot_tables(m.covariance_function_, fs)
        r = fit._nll(num_probes, seed, probes, None, slots, table, tangents)
        self.value_iterations, self.value_residual = r["iterations"], r["residual"]
        grad, stderr, by_name = self._gradient_by_name(slots, r["grad"], r["grad_stderr"], r["grad_samples"])
        out = (-r["nll"], r["nll_stderr"], grad, stderr)
        return out + (r["samples"], by_name) if return_samples else out

    def _gradient_by_name(self, slots, g, se, samples):
        """per name: the gradients of its slots add; a name with one slot keeps the entry's standard error, a shared name
        takes it from the summed samples of its slots; mean-function parameters are exact"""
        m, fit = self._model, self._fit
        t = samples.shape[0]
        grad = {name: 0. for name in m.get_params()}
        stderr = {name: 0. for name in m.get_params()}
        by_name, count = {}, {}
        for p, (_, _, name) in enumerate(slots):
            grad[name] -= g[p]
            by_name[name] = by_name.get(name, 0.) + samples[:, p]
            count[name] = count.get(name, 0) + 1
            stderr[name] = se[p]
        for name, sm in by_name.items():
            if count[name] > 1:
                tau = sm.sum() / t
                stderr[name] = 0.5 * np.sqrt(((sm - tau) ** 2).sum() / (t * (t - 1))) if t > 1 else float("nan")
        for name in m.mean_function_.get_params():
            grad[name] += float(m._mean_tangent(fit.feature_set, name) @ fit.information)
        return grad, stderr, by_name

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
    return IterativeFitModel(model, IterativeGPFit(ctx, h, fs.n, dataset.features, info, it.value, res.value, fs))
