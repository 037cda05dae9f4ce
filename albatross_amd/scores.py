"""Scores of a joint prediction against held-out truth (include/albatross/src/evaluation/prediction_metrics.hpp:
chi_squared_cdf :136-145, score::crps_normal :349-364, score::energy_score :387-435, score::variogram_score :465-520) and
draws from it (score::detail::draw_mvn :200-217), computed where the prediction lives.

`prediction` is anything with `.mean` and `.covariance` - a JointDistribution of numpy arrays or the
DeviceJointDistribution of `Prediction.joint(on_device=True)`; `truth` is an array or a MarginalDistribution, whose
variance joins the diagonal of the prediction's covariance as in the reference.  When any array argument is a
DeviceArray the call runs on device-resident data (host arrays among the arguments are uploaded) and nothing of size
m x m crosses the bus.  All arithmetic is in the HIP library (include/albatross_amd.h, "scoring a joint prediction").
"""
import ctypes as C
import math

import numpy as np

from . import _capi as capi
from .gp import DeviceArray, MarginalDistribution, default_context

ENERGY_SCORE_DEFAULT_SAMPLE_COUNT = 1000   # constant::cEnergyScoreDefaultSampleCount
ENERGY_SCORE_DEFAULT_SEED = 22             # constant::cEnergyScoreDefaultSeed
DEFAULT_VARIOGRAM_SCORE_ORDER = "madogram"  # constant::cDefaultVariogramScoreOrder
_ORDERS = {"madogram": 1, "variogram": 2, 1: 1, 2: 2}


class _Args:
    """the array arguments of one call, all at one location: AGP_DEVICE as soon as one of them is a DeviceArray"""

    def __init__(self, *arrays):
        dev = [a for a in arrays if isinstance(a, DeviceArray)]
        self.ctx = dev[0]._ctx if dev else default_context()
        self.location = capi.DEVICE if dev else capi.HOST
        self._keep = []

    def vector(self, a):
        if a is None:
            return None
        if isinstance(a, DeviceArray):
            return C.c_void_p(a.ptr)
        a = np.ascontiguousarray(a, dtype=np.float64)
        return self._place(a)

    def matrix(self, a):
        """column-major m x n; returns (pointer, leading dimension)"""
        if a is None:
            return None, 0
        if isinstance(a, DeviceArray):
            return C.c_void_p(a.ptr), a.shape[0]
        a = np.asfortranarray(a, dtype=np.float64)
        return self._place(a), a.shape[0]

    def _place(self, a):
        if self.location == capi.DEVICE:
            a = self.ctx.to_device(a.T if a.ndim == 2 else a)  # (to_device uploads C order: the transpose's is a's column-major)
            self._keep.append(a)
            return C.c_void_p(a.ptr)
        self._keep.append(a)
        return C.c_void_p(a.ctypes.data)


def _truth_parts(truth):
    if isinstance(truth, MarginalDistribution):
        return truth.mean, truth.covariance
    return truth, None


def _size(a):
    return int(a.shape[0])


def draw_mvn(joint, n_draws, seed=ENERGY_SCORE_DEFAULT_SEED, z=None):
    """detail::draw_mvn: `n_draws` samples of N(joint.mean, joint.covariance) as the columns of an m x n_draws matrix
    (numpy, or a DeviceArray for device-resident input), through the device LL^T of the covariance.  z (m x n_draws):
    the standard normals to use instead of the library's counter-based generator (agp_standard_normal)."""
    a = _Args(joint.mean, joint.covariance, z)
    ctx, lib, m = a.ctx, a.ctx._lib, _size(joint.mean)
    if tuple(joint.covariance.shape) != (m, m) or (z is not None and tuple(z.shape) != (m, n_draws)):
        raise ValueError("draw_mvn: sizes of mean, covariance and z do not match")
    cov, ldc = a.matrix(joint.covariance)
    zp, ldz = a.matrix(z)
    h = C.c_void_p()
    st = lib.agp_factor_create(ctx._h, cov, m, ldc, 0, a.location, C.byref(h))
    try:
        ctx._check(st, "agp_factor_create")
        if a.location == capi.DEVICE:
            out = ctx.device_empty((m, n_draws))
            dst = C.c_void_p(out.ptr)
        else:
            out = np.empty((m, n_draws), order="F")
            dst = C.c_void_p(out.ctypes.data)
        ctx._check(lib.agp_draw_mvn(ctx._h, h, a.vector(joint.mean), n_draws, seed, zp, ldz, dst, m, a.location), "agp_draw_mvn")
    finally:
        if h:
            lib.agp_fit_destroy(h)
    return out


def energy_score(prediction, truth, weights=None, seed=ENERGY_SCORE_DEFAULT_SEED, num_samples=ENERGY_SCORE_DEFAULT_SAMPLE_COUNT,
                 z=None):
    """score::energy_score: Monte-Carlo E||X - y|| - 0.5 E||X - X'|| with antithetic samples.  z (m x 2 (num_samples // 2 + 1)):
    the standard normals to use instead of the generator's."""
    y, yv = _truth_parts(truth)
    a = _Args(prediction.mean, prediction.covariance, y, yv, weights, z)
    m = _size(prediction.mean)
    if _size(y) != m or tuple(prediction.covariance.shape) != (m, m) or (weights is not None and _size(weights) != m):
        raise ValueError("energy_score: predictive distribution, truth and weights have different sizes")
    cov, ldc = a.matrix(prediction.covariance)
    zp, ldz = a.matrix(z)
    out = C.c_double()
    a.ctx._check(a.ctx._lib.agp_energy_score(a.ctx._h, a.vector(prediction.mean), cov, ldc, m, a.vector(y), a.vector(yv),
                                             a.vector(weights), seed, num_samples, zp, ldz, a.location, C.byref(out)),
                 "agp_energy_score")
    return out.value


def variogram_score(prediction, truth, weights=None, order=DEFAULT_VARIOGRAM_SCORE_ORDER):
    """score::variogram_score of order "madogram" (p = 1) or "variogram" (p = 2); weights: m x m, its strict upper
    triangle is what is read (the pairs i < j of the reference's loop)."""
    if order not in _ORDERS:
        raise ValueError("variogram_score: order is 'madogram' or 'variogram'")
    y, yv = _truth_parts(truth)
    a = _Args(prediction.mean, prediction.covariance, y, yv, weights)
    m = _size(prediction.mean)
    if _size(y) != m or tuple(prediction.covariance.shape) != (m, m) or (weights is not None and tuple(weights.shape) != (m, m)):
        raise ValueError("variogram_score: predictive distribution, truth and weights have different sizes")
    cov, ldc = a.matrix(prediction.covariance)
    w, ldw = a.matrix(weights)
    out = C.c_double()
    a.ctx._check(a.ctx._lib.agp_variogram_score(a.ctx._h, a.vector(prediction.mean), cov, ldc, m, a.vector(y), a.vector(yv), w, ldw,
                                                _ORDERS[order], a.location, C.byref(out)), "agp_variogram_score")
    return out.value


def crps_normal(mu, sigma, y):
    """score::crps_normal, elementwise; returns an array shaped like the broadcast arguments (a float for scalars)"""
    mu, sigma, y = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64),
                                       np.asarray(y, dtype=np.float64))
    ctx = default_context()
    flat = [np.ascontiguousarray(v).ravel() for v in (mu, sigma, y)]
    out = np.empty(flat[0].shape[0])
    ctx._check(ctx._lib.agp_crps_normal(ctx._h, *[C.c_void_p(v.ctypes.data) for v in flat], out.shape[0],
                                        C.c_void_p(out.ctypes.data), capi.HOST), "agp_crps_normal")
    return float(out[0]) if mu.ndim == 0 else out.reshape(mu.shape)


def _regularized_lower_gamma(a, x):
    """P(a, x) for a > 0, x >= 0: the series below a + 1, Lentz's continued fraction of Q above (the role of the
    reference's incomplete_gamma, stats/incomplete_gamma.hpp)"""
    if x <= 0.:
        return 0.
    log_front = a * math.log(x) - x - math.lgamma(a)
    if x < a + 1.:
        term = total = 1. / a
        n = a
        for _ in range(10000):
            n += 1.
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return min(1., total * math.exp(log_front))
    tiny = 1e-300
    b = x + 1. - a
    c, d = 1. / tiny, 1. / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1. / d
        delta = d * c
        h *= delta
        if abs(delta - 1.) < 1e-16:
            break
    return max(0., 1. - math.exp(log_front) * h)


def chi_squared_cdf_scalar(x, degrees_of_freedom):
    """chi_squared_cdf(x, dof), stats/chi_squared.hpp:29-67"""
    if math.isnan(x) or x < 0.:
        return math.nan
    if degrees_of_freedom == 0:
        return 1.
    if np.finfo(np.float64).eps > x:
        return 0.
    if math.isinf(x):
        return 1.
    return _regularized_lower_gamma(0.5 * degrees_of_freedom, 0.5 * x)


def chi_squared_cdf(prediction, truth):
    """chi_squared_cdf(prediction, truth) (prediction_metrics.hpp:136-141 -> stats/chi_squared.hpp:74-81): the quadratic
    form d^T (C + S)^-1 d through the device LL^T (factor + solve), its chi-squared CDF as a host scalar.  The deviation
    (m values) is formed on the host.  A device-resident covariance stays where it is unless the truth carries a
    variance: adding that diagonal needs a copy, which is then made on the host."""
    y, yv = _truth_parts(truth)
    mean = prediction.mean.numpy() if isinstance(prediction.mean, DeviceArray) else np.asarray(prediction.mean, dtype=np.float64)
    y = y.numpy() if isinstance(y, DeviceArray) else np.asarray(y, dtype=np.float64)
    m = _size(mean)
    if _size(y) != m or tuple(prediction.covariance.shape) != (m, m):
        raise ValueError("chi_squared_cdf: predictive distribution and truth have different sizes")
    deviation = np.ascontiguousarray(mean - y)
    cov = prediction.covariance
    if yv is not None:
        yv = yv.numpy() if isinstance(yv, DeviceArray) else np.asarray(yv, dtype=np.float64)
        cov = np.array(cov.numpy() if isinstance(cov, DeviceArray) else cov, dtype=np.float64, order="F")
        cov[np.diag_indices(m)] += yv
    a = _Args(cov)
    ctx, lib = a.ctx, a.ctx._lib
    covp, ldc = a.matrix(cov)
    h = C.c_void_p()
    st = lib.agp_factor_create(ctx._h, covp, m, ldc, 0, a.location, C.byref(h))
    try:
        ctx._check(st, "agp_factor_create")
        solved = np.empty(m)
        ctx._check(lib.agp_solve(ctx._h, h, C.c_void_p(deviation.ctypes.data), 1, C.c_void_p(solved.ctypes.data), capi.HOST),
                   "agp_solve")
    finally:
        if h:
            lib.agp_fit_destroy(h)
    return chi_squared_cdf_scalar(float(deviation @ solved), m)
