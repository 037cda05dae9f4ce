"""Host-side mirror of albatross's GaussianProcessRegression call surface.

Mirrors include/albatross/src/models/gp.hpp (GaussianProcessBase :170-463,
GaussianProcessRegression :487-505, factories :507-537), core/model.hpp,
core/fit_model.hpp and core/prediction.hpp: `gp_from_covariance(cov).fit(dataset)
.predict(features).mean()/.marginal()/.joint()`, `model.log_likelihood(dataset)`.
Every Gram / factor / solve / predict goes through the C-ABI in
include/albatross_amd.h (HIP kernels); nothing is computed on the CPU here.
"""
import ctypes as C
import itertools

import numpy as np

from . import _capi as capi
from .covariance import (CovarianceFunction, FeatureSet, LinearCombination, Measurement, expand_linear_combinations,
                         expand_with_offsets, has_linear_combinations, nodes_to_array)


class AlbatrossAmdError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        name = capi.load().agp_status_string(status).decode()
        super().__init__(f"albatross_amd: {name}" + (f" ({detail})" if detail else ""))


class NotPositiveDefiniteError(AlbatrossAmdError):
    pass


class NanInputError(AlbatrossAmdError):
    pass


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Context:
    """agp_context: HIP streams + workspaces of one GPU."""

    def __init__(self, device_id=0):
        self._lib = capi.load()
        h = C.c_void_p()
        st = self._lib.agp_context_create(device_id, C.byref(h))
        if st != capi.AGP_OK:
            raise AlbatrossAmdError(st, "agp_context_create")
        self._h = h
        self.device_id = device_id
        self._kernels = {}

    def close(self):
        if getattr(self, "_h", None):
            for kh in self._kernels.values():
                self._lib.agp_kernel_destroy(kh)
            self._kernels = {}
            self._lib.agp_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- helpers ---------------------------------------------------------------
    def _check(self, st, what):
        if st == capi.AGP_OK:
            return
        detail = what
        if st == capi.AGP_ERR_HIP:
            detail += ": " + self._lib.agp_last_error(self._h).decode()
        if st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE:
            raise NotPositiveDefiniteError(st, detail)
        if st == capi.AGP_ERR_NAN_INPUT:
            raise NanInputError(st, detail)
        raise AlbatrossAmdError(st, detail)

    def kernel(self, cov):
        """agp_kernel for the CURRENT parameter values of `cov` (cached by the
        flattened program bytes, so a tuner revisiting parameters re-uses it)."""
        nodes = cov.program_nodes()
        arr = nodes_to_array(nodes)
        key = bytes(arr)
        kh = self._kernels.pop(key, None)
        if kh is None:
            kh = C.c_void_p()
            self._check(self._lib.agp_kernel_create(arr, len(nodes), C.byref(kh)), "agp_kernel_create")
            # least-recently-used eviction, ONE entry at a time: a handle returned by this method stays valid for
            # the next KERNEL_CACHE - 1 calls at least (callers that collect more handles than that before using
            # them make private ones, see private_kernel)
            while len(self._kernels) >= self.KERNEL_CACHE:
                oldest = next(iter(self._kernels))
                self._lib.agp_kernel_destroy(self._kernels.pop(oldest))
        self._kernels[key] = kh  # (re-)inserted last = most recently used
        return kh

    KERNEL_CACHE = 64

    def private_kernel(self, cov):
        """an agp_kernel the CALLER owns (agp_kernel_destroy when done): outside the cache, never evicted"""
        nodes = cov.program_nodes()
        kh = C.c_void_p()
        self._check(self._lib.agp_kernel_create(nodes_to_array(nodes), len(nodes), C.byref(kh)), "agp_kernel_create")
        return kh

    def synchronize(self):
        """waits for everything queued on any of the context's streams (device-wide)"""
        self._check(self._lib.agp_context_synchronize(self._h), "synchronize")

    def to_device(self, array):
        """a DeviceArray holding a copy of `array` (fp64 / int64 numpy) in this context's HBM: what AGP_DEVICE arguments
        point at (agp_device_malloc + agp_memcpy; no second HIP runtime in the process)"""
        a = np.ascontiguousarray(array)
        d = DeviceArray(self, a.nbytes, a.dtype, a.shape)
        self._check(self._lib.agp_memcpy(self._h, C.c_void_p(d.ptr), C.c_void_p(a.ctypes.data), a.nbytes, capi.DEVICE), "agp_memcpy")
        return d

    def device_empty(self, shape, dtype=np.float64):
        shape = tuple(np.atleast_1d(shape).astype(np.int64).tolist())
        return DeviceArray(self, int(np.prod(shape)) * np.dtype(dtype).itemsize, np.dtype(dtype), shape)

    def set_profiling(self, enabled):
        self._check(self._lib.agp_set_profiling(self._h, 1 if enabled else 0), "set_profiling")

    def stage_ms(self, stage):
        v = C.c_double()
        self._check(self._lib.agp_last_stage_ms(self._h, stage, C.byref(v)), "last_stage_ms")
        return v.value

    def gram(self, cov, xs, ys=None):
        """compute_covariance_matrix (callers.hpp:38-166) on the device."""
        if has_linear_combinations(xs) or (ys is not None and has_linear_combinations(ys)):
            # LinearCombinationCaller (callers.hpp:321-396): Gram of the expanded points AND its contraction with the
            # coefficients on the device (agp_gram_combined)
            ex, xoff, xc = expand_with_offsets(xs)
            fx = cov.features(ex)
            sx = fx.as_struct()
            kh = self.kernel(cov)
            nx = len(xoff) - 1
            if ys is None:
                out = np.empty((nx, nx), order="F")
                st = self._lib.agp_gram_combined(self._h, kh, C.byref(sx), nx, _ptr(xoff), _ptr(xc), None, 0, None, None,
                                                 _ptr(out), max(nx, 1), capi.HOST)
            else:
                ey, yoff, yc = expand_with_offsets(ys)
                fy = cov.features(ey)
                sy = fy.as_struct()
                ny = len(yoff) - 1
                out = np.empty((nx, ny), order="F")
                st = self._lib.agp_gram_combined(self._h, kh, C.byref(sx), nx, _ptr(xoff), _ptr(xc), C.byref(sy), ny, _ptr(yoff),
                                                 _ptr(yc), _ptr(out), max(nx, 1), capi.HOST)
            self._check(st, "agp_gram_combined")
            return out
        fx = cov.features(xs)
        sx = fx.as_struct()
        kh = self.kernel(cov)
        if ys is None:
            out = np.empty((fx.n, fx.n), order="F")
            st = self._lib.agp_gram(self._h, kh, C.byref(sx), None, _ptr(out), max(fx.n, 1), capi.HOST)
        else:
            fy = cov.features(ys)
            sy = fy.as_struct()
            out = np.empty((fx.n, fy.n), order="F")
            st = self._lib.agp_gram(self._h, kh, C.byref(sx), C.byref(sy), _ptr(out), max(fx.n, 1), capi.HOST)
        self._check(st, "agp_gram")
        return out

    def gram_diagonal(self, cov, xs):
        if has_linear_combinations(xs):
            return np.diag(self.gram(cov, xs)).copy()
        f = cov.features(xs)
        return np.array([self.gram(cov, FeatureSet(f.coords[i:i + 1],
                                                   None if f.scales is None else list(f.scales[i:i + 1].T),
                                                   None if f.eq_id is None else f.eq_id[i:i + 1],
                                                   f.is_measurement))[0, 0] for i in range(f.n)])


_default_context = None


class DeviceArray:
    """`nbytes` of device memory owned by a Context (agp_device_malloc); `.ptr` is the integer device address that the
    AGP_DEVICE arguments of the C-ABI take, `.numpy()` downloads (after the context's streams have drained)."""

    def __init__(self, ctx, nbytes, dtype=np.float64, shape=None):
        self._ctx = ctx
        self.nbytes = int(nbytes)
        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape) if shape is not None else (self.nbytes // self.dtype.itemsize,)
        p = C.c_void_p()
        ctx._check(ctx._lib.agp_device_malloc(ctx._h, max(self.nbytes, 8), C.byref(p)), "agp_device_malloc")
        self.ptr = p.value

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        self._ctx._check(self._ctx._lib.agp_memcpy(self._ctx._h, C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), self.nbytes, capi.HOST),
                         "agp_memcpy")
        return out

    def free(self):
        if getattr(self, "ptr", None) and getattr(self._ctx, "_h", None):
            self._ctx._lib.agp_device_free(self._ctx._h, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def default_context():
    global _default_context
    if _default_context is None:
        _default_context = Context(0)
    return _default_context


# ---------------------------------------------------------------------------
# core containers (core/dataset.hpp, core/distribution.hpp)
# ---------------------------------------------------------------------------
class MarginalDistribution:
    """mean + diagonal covariance (core/distribution.hpp)."""

    def __init__(self, mean, covariance=None):
        self.mean = np.asarray(mean, dtype=np.float64)
        self.covariance = None if covariance is None else np.asarray(covariance, dtype=np.float64)

    def size(self):
        return self.mean.shape[0]


class JointDistribution:
    def __init__(self, mean, covariance):
        self.mean = np.asarray(mean, dtype=np.float64)
        self.covariance = np.asarray(covariance, dtype=np.float64)

    def size(self):
        return self.mean.shape[0]

    def marginal(self):
        return MarginalDistribution(self.mean, np.diag(self.covariance).copy())


class DeviceJointDistribution:
    """A JointDistribution left in HBM: `mean` (m) and `covariance` (m x m, column-major) are DeviceArrays - what
    `Prediction.joint(on_device=True)` returns and the scores of albatross_amd.scores take as they are."""

    def __init__(self, mean, covariance):
        self.mean = mean
        self.covariance = covariance

    def size(self):
        return self.mean.shape[0]

    def numpy(self):
        m = self.size()
        return JointDistribution(self.mean.numpy(), self.covariance.numpy().ravel().reshape((m, m), order="F"))  # the bytes are column-major


class RegressionDataset:
    """RegressionDataset<Feature>{features, targets} (core/dataset.hpp)."""

    def __init__(self, features, targets):
        self.features = features
        if not isinstance(targets, MarginalDistribution):
            targets = MarginalDistribution(targets)
        self.targets = targets

    def size(self):
        return self.targets.size()


class MeanFunction:
    """MeanFunction<Derived> (covariance_functions/mean_function.hpp:18-134): `m(coords)` is the mean vector
    (operator()(std::vector<X>), :73-84); `+` / `*` compose (:136-271).  `nodes()` is the function flattened to
    postfix tuples ("zero",) / ("linear", slope, offset) / ("sum",) / ("product",), like get_name() a description."""

    def get_params(self):
        return {}

    def set_param(self, name, value):
        raise KeyError(name)

    def __add__(self, other):
        return SumOfMeanFunctions(self, other)

    def __mul__(self, other):
        return ProductOfMeanFunctions(self, other)


class ZeroMean(MeanFunction):
    """mean_function.hpp:274-276"""

    def __call__(self, coords):
        return np.zeros(len(coords))

    def nodes(self):
        return [("zero",)]


class LinearMean(MeanFunction):
    """slope * x + offset on 1-D features (polynomials.hpp:92-106)."""

    def __init__(self, slope=0., offset=0.):
        self._params = {"slope": float(slope), "offset": float(offset)}

    def get_params(self):
        return dict(self._params)

    def set_param(self, name, value):
        if name not in self._params:
            raise KeyError(name)
        self._params[name] = float(value)

    def __call__(self, coords):
        x = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)[:, 0]
        return self._params["slope"] * x + self._params["offset"]

    def nodes(self):
        return [("linear", self._params["slope"], self._params["offset"])]


class _BinaryMean(MeanFunction):
    def __init__(self, lhs, rhs):
        self.lhs_, self.rhs_ = lhs, rhs

    def get_params(self):  # map_join(lhs_.get_params(), rhs_.get_params())
        out = dict(self.lhs_.get_params())
        out.update(self.rhs_.get_params())
        return out

    def set_param(self, name, value):  # set_param_if_exists_in_any
        done = False
        for side in (self.lhs_, self.rhs_):
            if name in side.get_params():
                side.set_param(name, value)
                done = True
        if not done:
            raise KeyError(name)


class SumOfMeanFunctions(_BinaryMean):
    """mean_function.hpp:136-190"""

    def __call__(self, coords):
        return self.lhs_(coords) + self.rhs_(coords)

    def nodes(self):
        return self.lhs_.nodes() + self.rhs_.nodes() + [("sum",)]


class ProductOfMeanFunctions(_BinaryMean):
    """mean_function.hpp:192-260: lhs * rhs with rhs skipped where lhs == 0 (:221-227)"""

    def __call__(self, coords):
        out = np.array(self.lhs_(coords), dtype=np.float64)
        nz = out != 0.
        if nz.any():
            out[nz] *= np.asarray(self.rhs_(coords), dtype=np.float64)[nz]
        return out

    def nodes(self):
        return self.lhs_.nodes() + self.rhs_.nodes() + [("product",)]


def _values_of(features):
    return features.values if isinstance(features, Measurement) else features


def _mean_at(mean_function, cov, features):
    """mean_function(features) including LinearCombination features: sum_i a_i m(x_i) (callers.hpp:386-396)"""
    if has_linear_combinations(features):
        ex, Cx = expand_linear_combinations(_values_of(features))
        return Cx.T @ mean_function(np.asarray(ex, dtype=np.float64))
    return mean_function(cov.features(features).coords)


# ---------------------------------------------------------------------------
# Fit<GPFit<...>> (gp.hpp:43-77): device factor + information vector
# ---------------------------------------------------------------------------
class _DeviceSolver:
    """A CovarianceRepresentation that lives on the device as an `agp_solver` (include/albatross_amd.h): the handle is made on
    first use and goes with the object.  Subclasses provide `_make_solver()`."""
    _sv = None

    def _solver(self):
        if self._sv is None:
            self._sv = self._make_solver()
        return self._sv

    def _drop_solver(self):
        try:
            if getattr(self, "_sv", None) and self._ctx._h:
                self._ctx._lib.agp_solver_destroy(self._sv)
        except Exception:
            pass
        self._sv = None

    def _solve_through_handle(self, rhs):
        rhs = np.asarray(rhs, dtype=np.float64)
        r2 = np.asfortranarray(rhs.reshape(rhs.shape[0], -1))
        out = np.empty_like(r2, order="F")
        self._ctx._check(self._ctx._lib.agp_solver_solve(self._ctx._h, self._solver(), _ptr(r2), r2.shape[1], _ptr(out), capi.HOST),
                         "agp_solver_solve")
        return out.reshape(rhs.shape, order="F")


class GPFit(_DeviceSolver):

    def _make_solver(self):
        h = C.c_void_p()
        self._ctx._check(self._ctx._lib.agp_solver_from_fit(self._ctx._h, self._h, C.byref(h)), "agp_solver_from_fit")
        return h

    def __init__(self, ctx, handle, n, train_features):
        self._ctx = ctx
        self._h = handle
        self.n = n
        self.train_features = train_features
        self._information = None

    def __del__(self):
        self._drop_solver()
        try:
            if getattr(self, "_h", None) and self._ctx._h:
                self._ctx._lib.agp_fit_destroy(self._h)
            self._h = None
        except Exception:
            pass

    @property
    def information(self):
        if self._information is None:
            out = np.empty(self.n)
            self._ctx._check(self._ctx._lib.agp_fit_download_information(self._ctx._h, self._h, _ptr(out)),
                             "download_information")
            self._information = out
        return self._information

    # a mixed-precision factor (agp_fit_create_mixed): its log-determinant carries the rounding of the bulk products.
    # MEASURED (include/albatross_amd.h; tests/test_full_size_configs_gpu.py holds each figure): default fp16 x 2 path 0.5e-6 N
    # on BASELINE config 4's covariance at N = 32768, 1.9e-6 N on config 3's kernel - inside the 2e-6 N log-likelihood bar,
    # the latter just; bf16 x 3 (AGP_MIXED_F16=0) 0.8e-6 N / 4.3e-6 N; fp32 fallback (AGP_MIXED_BF16=0) 1.3e-5 relative.
    # The bound depends on the covariance function and is not proven for an arbitrary one, so reading it stays an explicit opt-in.
    mixed_precision = False
    accept_mixed_log_determinant = False

    @property
    def log_determinant(self):
        if self.mixed_precision and not self.accept_mixed_log_determinant:
            raise AlbatrossAmdError(capi.AGP_ERR_UNSUPPORTED,
                                    "log_determinant of a mixed-precision factor carries the rounding of the bulk products "
                                    "(measured 0.5e-6 N ... 1.9e-6 N on the default fp16 x 2 path, up to 4.9e-6 N on bf16 x 3, 1.9e-5 N on the fp32 "
                                    "fallback; whether that meets the 2e-6 N bar depends on the covariance function): use model.log_likelihood "
                                    "(always fp64) or set fit.accept_mixed_log_determinant = True")
        v = C.c_double()
        self._ctx._check(self._ctx._lib.agp_fit_log_determinant(self._h, C.byref(v)), "log_determinant")
        return v.value

    def rows(self):
        return self.n

    def solve(self, rhs):
        """train_covariance.solve(rhs) (CovarianceRepresentation, gp.hpp:42-45)."""
        rhs = np.asarray(rhs, dtype=np.float64)
        b = np.asfortranarray(rhs.reshape(self.n, -1, order="F"))
        out = np.empty_like(b, order="F")
        self._ctx._check(self._ctx._lib.agp_solve(self._ctx._h, self._h, _ptr(b), b.shape[1], _ptr(out), capi.HOST),
                         "agp_solve")
        return out.reshape(rhs.shape, order="F")

    def inverse_diagonal(self):
        """SerializableLDLT::inverse_diagonal (serializable_ldlt.hpp:181-199)."""
        out = np.empty(self.n)
        self._ctx._check(self._ctx._lib.agp_fit_inverse_diagonal(self._ctx._h, self._h, _ptr(out), capi.HOST),
                         "agp_fit_inverse_diagonal")
        return out

    def leave_one_out(self, target_mean):
        """Leave-one-out predictive marginals of every training point
        (held_out_predictions with singleton groups, cross_validation_utils.hpp:165-232)."""
        y = np.ascontiguousarray(target_mean, dtype=np.float64)
        mean, var = np.empty(self.n), np.empty(self.n)
        self._ctx._check(self._ctx._lib.agp_loo_marginal(self._ctx._h, self._h, _ptr(y), _ptr(mean), _ptr(var),
                                                         capi.HOST), "agp_loo_marginal")
        return MarginalDistribution(mean, var)

    @staticmethod
    def _flatten_groups(groups, n):
        offsets = np.zeros(len(groups) + 1, dtype=np.int64)
        if len(groups):
            offsets[1:] = np.cumsum([len(g) for g in groups])
        parts = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
        indices = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
        if indices.size and (indices.min() < 0 or indices.max() >= n):
            raise IndexError("group index out of range")
        return offsets, indices

    def inverse_blocks(self, groups):
        """SerializableLDLT::inverse_blocks (serializable_ldlt.hpp:137-179): [(K^-1)[I_g, I_g] for g in groups]."""
        offsets, indices = self._flatten_groups(groups, self.n)
        out = np.empty(int(sum(len(g) ** 2 for g in groups)))
        self._ctx._check(self._ctx._lib.agp_fit_inverse_blocks(self._ctx._h, self._h, len(groups), _ptr(offsets),
                                                               _ptr(indices), _ptr(out), capi.HOST),
                         "agp_fit_inverse_blocks")
        blocks, pos = [], 0
        for g in groups:
            m = len(g)
            blocks.append(out[pos:pos + m * m].reshape(m, m, order="F").copy())
            pos += m * m
        return blocks

    def held_out_predictions(self, target_mean, groups, joint=False):
        """details::held_out_predictions (cross_validation_utils.hpp:165-232): for every index group the
        prediction of its targets from all other groups, without refitting.  Returns one
        MarginalDistribution (joint=False) or JointDistribution (joint=True) per group."""
        y = np.ascontiguousarray(target_mean, dtype=np.float64)
        if y.shape[0] != self.n:
            raise ValueError("target size")
        offsets, indices = self._flatten_groups(groups, self.n)
        total = int(offsets[-1])
        mean, var = np.empty(total), np.empty(total)
        jb = np.empty(int(sum(len(g) ** 2 for g in groups))) if joint else None
        self._ctx._check(self._ctx._lib.agp_held_out_predictions(
            self._ctx._h, self._h, _ptr(y), len(groups), _ptr(offsets), _ptr(indices), _ptr(mean), _ptr(var),
            _ptr(jb), capi.HOST), "agp_held_out_predictions")
        out, pos = [], 0
        for gi, g in enumerate(groups):
            m, o = len(g), int(offsets[gi])
            if joint:
                out.append(JointDistribution(mean[o:o + m].copy(), jb[pos:pos + m * m].reshape(m, m, order="F").copy()))
                pos += m * m
            else:
                out.append(MarginalDistribution(mean[o:o + m].copy(), var[o:o + m].copy()))
        return out

    def factor(self):
        L = np.empty((self.n, self.n), order="F")
        self._ctx._check(self._ctx._lib.agp_fit_download_factor(self._ctx._h, self._h, _ptr(L), self.n),
                         "download_factor")
        return L


class DenseFactor(_DeviceSolver):
    """`Eigen::SerializableLDLT(const MatrixXd &)` (eigen/serializable_ldlt.hpp:27): the
    device LL^T of a dense symmetric positive-definite matrix (lower triangle read)."""
    _make_solver = GPFit._make_solver

    def __init__(self, matrix, context=None):
        self._ctx = context or default_context()
        K = np.asarray(matrix, dtype=np.float64)
        if K.ndim != 2 or K.shape[0] != K.shape[1]:
            raise ValueError("square matrix expected")
        if not (K.flags.f_contiguous or K.flags.c_contiguous):
            K = np.asfortranarray(K)
        # the LOWER triangle of the array is what is read.  A C-ordered (row-major) array seen
        # column-major is its transpose, whose UPPER triangle that is: no host copy, uplo = 1.
        uplo = 0 if K.flags.f_contiguous else 1
        self.n = K.shape[0]
        h = C.c_void_p()
        st = self._ctx._lib.agp_factor_create(self._ctx._h, _ptr(K), self.n, self.n, uplo, capi.HOST, C.byref(h))
        if st != capi.AGP_OK:
            pivot = self._ctx._lib.agp_fit_failed_pivot(h) if h else -1
            if h:
                self._ctx._lib.agp_fit_destroy(h)
            self._ctx._check(st, f"agp_factor_create (pivot {pivot})")
        self._h = h

    def __del__(self):
        self._drop_solver()
        try:
            if getattr(self, "_h", None) and self._ctx._h:
                self._ctx._lib.agp_fit_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def rows(self):
        return self.n

    solve = GPFit.solve
    inverse_diagonal = GPFit.inverse_diagonal
    factor = GPFit.factor
    mixed_precision = False  # (always an fp64 factor)
    log_determinant = GPFit.log_determinant


class PivotedLDLT(_DeviceSolver):
    """Eigen::LDLT<MatrixXd, Lower> as SerializableLDLT wraps it (eigen/serializable_ldlt.hpp:27): the
    diagonally pivoted P A P^T = L D L^T on the device, for symmetric matrices that are only semi-definite
    (the un-pivoted DenseFactor rejects those).  Same operation order as the reference's unblocked
    algorithm: matrix_ldlt(), vector_d() and transpositions() are bit-identical to the CPU restatement."""

    def __init__(self, matrix, context=None):
        self._ctx = context or default_context()
        K = np.asarray(matrix, dtype=np.float64)
        if K.ndim != 2 or K.shape[0] != K.shape[1]:
            raise ValueError("square matrix expected")
        if not (K.flags.f_contiguous or K.flags.c_contiguous):
            K = np.asfortranarray(K)
        uplo = 0 if K.flags.f_contiguous else 1  # lower triangle of the array, whatever its memory order
        self.n = K.shape[0]
        h, ok = C.c_void_p(), C.c_int(1)
        self._ctx._check(self._ctx._lib.agp_ldlt_create(self._ctx._h, _ptr(K), self.n, self.n, uplo, capi.HOST,
                                                        C.byref(h), C.byref(ok)), "agp_ldlt_create")
        self._h = h
        self.success = bool(ok.value)  # info() == Eigen::Success

    def _make_solver(self):
        h = C.c_void_p()
        self._ctx._check(self._ctx._lib.agp_solver_from_ldlt(self._ctx._h, self._h, C.byref(h)), "agp_solver_from_ldlt")
        return h

    def __del__(self):
        self._drop_solver()
        try:
            if getattr(self, "_h", None) and self._ctx._h:
                self._ctx._lib.agp_ldlt_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def rows(self):
        return self.n

    def solve(self, rhs):
        """LDLT::solve: P^T L^-T D^+ L^-1 P rhs."""
        rhs = np.asarray(rhs, dtype=np.float64)
        r2 = np.asfortranarray(rhs.reshape(rhs.shape[0], -1))
        out = np.empty_like(r2, order="F")
        self._ctx._check(self._ctx._lib.agp_ldlt_solve(self._ctx._h, self._h, _ptr(r2), r2.shape[1], _ptr(out),
                                                       capi.HOST), "agp_ldlt_solve")
        return out.reshape(rhs.shape, order="F")

    def sqrt_solve(self, rhs):
        """SerializableLDLT::sqrt_solve (:99-109): D^-1/2 L^-1 P rhs."""
        rhs = np.asarray(rhs, dtype=np.float64)
        r2 = np.asfortranarray(rhs.reshape(rhs.shape[0], -1))
        out = np.empty_like(r2, order="F")
        self._ctx._check(self._ctx._lib.agp_ldlt_sqrt_solve(self._ctx._h, self._h, _ptr(r2), r2.shape[1], _ptr(out),
                                                            capi.HOST), "agp_ldlt_sqrt_solve")
        return out.reshape(rhs.shape, order="F")

    def vector_d(self):
        d = np.empty(self.n)
        self._ctx._check(self._ctx._lib.agp_ldlt_vector_d(self._h, _ptr(d)), "agp_ldlt_vector_d")
        return d

    def transpositions(self):
        tr = np.empty(self.n, dtype=np.int64)
        self._ctx._check(self._ctx._lib.agp_ldlt_transpositions(self._h, _ptr(tr)), "agp_ldlt_transpositions")
        return tr

    def matrix_ldlt(self):
        out = np.empty((self.n, self.n), order="F")
        self._ctx._check(self._ctx._lib.agp_ldlt_download(self._ctx._h, self._h, _ptr(out), self.n), "agp_ldlt_download")
        return out

    @property
    def log_determinant(self):
        """serializable_ldlt.hpp:128-135: sum(log(vectorD)) (NaN / -inf for non-positive pivots, like the reference)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.log(self.vector_d()).sum())


def negative_log_likelihood(deviation, covariance, context=None):
    """negative_log_likelihood(deviation, covariance) (evaluation/likelihood.hpp:53-66)."""
    ctx = context or default_context()
    d = np.ascontiguousarray(deviation, dtype=np.float64)
    K = np.asarray(covariance, dtype=np.float64)
    if not (K.flags.f_contiguous or K.flags.c_contiguous):
        K = np.asfortranarray(K)
    uplo = 0 if K.flags.f_contiguous else 1
    out = C.c_double()
    ctx._check(ctx._lib.agp_nll_dense(ctx._h, _ptr(d), _ptr(K), d.shape[0], K.shape[0], uplo, capi.HOST,
                                      C.byref(out)), "agp_nll_dense")
    return out.value


class BlockSymmetric(_DeviceSolver):
    """linalg/block_symmetric.hpp:46-115: solver of [[A, B], [B^T, C]] from a solver of A, Ai_B = A^-1 B and the factor of
    the Schur complement S = C - B^T A^-1 B - ON THE DEVICE (agp_solver_block_symmetric): Ai_B is computed and kept in HBM,
    a solve is device solves + MFMA products.  Only solvers that are not a plain device factor end up here (pivoted
    LDL^T fits, fit_from_prediction); fits on the device factor are updated by agp_fit_update."""

    def __init__(self, A, B, S):
        self._ctx = A._ctx
        self.A, self.S = A, S  # (kept alive: the device object borrows their solvers)
        self._B = np.asfortranarray(B, dtype=np.float64)
        if self._B.shape != (A.rows(), S.rows()):
            raise ValueError("BlockSymmetric: B must be rows(A) x rows(S)")

    def _make_solver(self):
        h = C.c_void_p()
        self._ctx._check(self._ctx._lib.agp_solver_block_symmetric(self._ctx._h, self.A._solver(), _ptr(self._B), self._B.shape[0], capi.HOST,
                                                                   self.S._solver(), C.byref(h)), "agp_solver_block_symmetric")
        return h

    def __del__(self):
        self._drop_solver()

    def rows(self):
        return self.A.rows() + self.S.rows()

    def solve(self, rhs):  # block_symmetric.hpp:75-98
        return self._solve_through_handle(rhs)

    def update_information(self, information, si_delta):
        """gp.hpp:403-407: [information - Ai_B Si_delta ; Si_delta] from the Ai_B this solver holds in HBM
        (agp_solver_update_information: one mat-vec on the device)."""
        info = np.ascontiguousarray(information, dtype=np.float64)
        sd = np.ascontiguousarray(si_delta, dtype=np.float64)
        out = np.empty(info.shape[0] + sd.shape[0])
        self._ctx._check(self._ctx._lib.agp_solver_update_information(self._ctx._h, self._solver(), _ptr(info), _ptr(sd), _ptr(out), capi.HOST),
                         "agp_solver_update_information")
        return out


class ExplainedCovariance(_DeviceSolver):
    """ExplainedCovariance (covariance_functions/representations.hpp:64-96): S^-1 = A^-1 B A^-1 with the outer matrix A
    held through its factor and the inner matrix B kept as it is, because B may be singular - on the device
    (agp_solver_explained): the product with B between the two solves is an MFMA product in HBM."""

    def __init__(self, outer, inner, context=None):
        self.outer_ldlt = outer if isinstance(outer, (DenseFactor, PivotedLDLT)) else DenseFactor(outer, context)
        self._ctx = self.outer_ldlt._ctx
        self.inner = np.asfortranarray(inner, dtype=np.float64)

    def _make_solver(self):
        h = C.c_void_p()
        self._ctx._check(self._ctx._lib.agp_solver_explained(self._ctx._h, self.outer_ldlt._solver(), _ptr(self.inner), self.inner.shape[0],
                                                             capi.HOST, C.byref(h)), "agp_solver_explained")
        return h

    def __del__(self):
        self._drop_solver()

    def rows(self):
        return self.inner.shape[0]

    def solve(self, rhs):  # representations.hpp:80-82
        return self._solve_through_handle(rhs)


class UpdatedGPFit:
    """Fit<GPFit<Representation, F>> whose solver is not the plain LL^T factor: a pivoted L D L^T (semi-definite covariances),
    BlockSymmetric<Solver> from update() (gp.hpp:384-414) or ExplainedCovariance from fit_from_prediction (gp.hpp:139-153).
    The solver is a device object (`agp_solver`) and predictions go through agp_solver_predict - the generic
    CovarianceRepresentation form of _predict_impl (gp.hpp:305-366) in HBM - agp_solver_predict_combined when either side holds
    LinearCombination features (their covariance matrices are built and contracted on the device too)."""

    def __init__(self, train_features, train_covariance, information):
        self.train_features = train_features
        self.train_covariance = train_covariance
        self.information = information
        self.n = information.shape[0]

    def rows(self):
        return self.n

    def solve(self, rhs):
        return self.train_covariance.solve(rhs)


class Prediction:
    """Lazy prediction object (core/prediction.hpp:115-224)."""

    def __init__(self, fit_model, features):
        self._fm = fit_model
        self._features = features

    def mean(self):
        return self._fm._predict_mean(self._features)

    def marginal(self):
        return self._fm._predict_marginal(self._features)

    def joint(self, on_device=False):
        """on_device=True: a DeviceJointDistribution - the m x m covariance stays in HBM (plain LL^T fits only)"""
        if on_device:
            return self._fm._predict_joint_on_device(self._features)
        return self._fm._predict_joint(self._features)


class FitModel:
    """FitModel<Model, Fit> (core/fit_model.hpp:18-114)."""

    def __init__(self, model, fit):
        self._model = model
        self._fit = fit

    def get_fit(self):
        return self._fit

    def get_model(self):
        return self._model

    def predict(self, features):
        return Prediction(self, features)

    def predict_with_measurement_noise(self, features):
        """fit_model.hpp:54-62: wraps the test features in Measurement<>."""
        return Prediction(self, features if isinstance(features, Measurement) else Measurement(features))

    def update(self, dataset, targets=None):
        """FitModel::update (core/fit_model.hpp:68-81) -> _update_impl (gp.hpp:384-414):
        condition the fit on further observations through the Schur complement instead of
        re-factoring; returns a new FitModel whose fit holds a BlockSymmetric solver."""
        if targets is not None:
            dataset = RegressionDataset(dataset, targets)
        m, ctx = self._model, self._model._ctx()
        feats = _values_of(dataset.features)
        if isinstance(self._fit, GPFit) and not has_linear_combinations(feats):
            return self._update_on_device(dataset, feats)
        pred = self.predict(feats).joint()                                   # gp.hpp:388-389
        delta = np.asarray(dataset.targets.mean, dtype=np.float64) - pred.mean
        S = np.array(pred.covariance)
        if dataset.targets.covariance is not None:
            S[np.diag_indices_from(S)] += dataset.targets.covariance         # pred.covariance += targets.covariance
        S_ldlt = DenseFactor(S, ctx)                                          # gp.hpp:393
        old_feats = _values_of(self._fit.train_features)
        cross = ctx.gram(m.covariance_function_, old_feats, feats)            # gp.hpp:395-396
        solver_a = self._fit.train_covariance if isinstance(self._fit, UpdatedGPFit) else self._fit
        new_cov = BlockSymmetric(solver_a, cross, S_ldlt)                     # gp.hpp:398-399
        Si_delta = S_ldlt.solve(delta)
        info = new_cov.update_information(self._fit.information, Si_delta)   # gp.hpp:403-407, on the device
        new_feats = np.concatenate([np.asarray(old_feats, dtype=np.float64).reshape(self._fit.rows(), -1),
                                    np.asarray(feats, dtype=np.float64).reshape(len(delta), -1)])
        return FitModel(m, UpdatedGPFit(new_feats, new_cov, info))

    def _update_on_device(self, dataset, feats):
        """agp_fit_update: the resident factor grows by one block row (V^T = (L^-1 B)^T, L_S from the Schur complement);
        triangular solve, SYRK, LL^T of the new block and the back substitution all run in the HIP library."""
        m, ctx = self._model, self._model._ctx()
        cov = m.covariance_function_
        fs = cov.features(feats)
        y, yv = m._targets(fs, dataset.targets)      # mean function removed (ModelBase::update -> remove_from)
        s = fs.as_struct()
        h = C.c_void_p()
        st = ctx._lib.agp_fit_update(ctx._h, ctx.kernel(cov), self._fit._h, C.byref(s), _ptr(y), _ptr(yv), C.byref(h), None, None)
        if st != capi.AGP_OK:
            pivot = ctx._lib.agp_fit_failed_pivot(h) if h else -1
            if h:
                ctx._lib.agp_fit_destroy(h)
            ctx._check(st, f"agp_fit_update (pivot {pivot})")
        old_feats = _values_of(self._fit.train_features)
        try:
            new_feats = np.concatenate([np.asarray(old_feats, dtype=np.float64).reshape(self._fit.rows(), -1),
                                        np.asarray(feats, dtype=np.float64).reshape(fs.n, -1)])
        except (TypeError, ValueError):  # feature containers numpy cannot stack: keep them side by side
            new_feats = (old_feats, feats)
        return FitModel(m, GPFit(ctx, h, self._fit.rows() + fs.n, new_feats))

    # --- _predict_impl (gp.hpp:305-366) ------------------------------------------
    def _host_predict(self, features, want):
        """_predict_impl written against a generic CovarianceRepresentation (gp.hpp:305-366), for fits whose solver is not the
        plain LL^T factor: agp_solver_predict - cross covariance, solve, explained covariance all in HBM."""
        m, ctx = self._model, self._model._ctx()
        cov = m.covariance_function_
        if not (has_linear_combinations(features) or has_linear_combinations(self._fit.train_features)):
            fs = cov.features(features)
            ftr = cov.features(self._fit.train_features)
            s_xs, s_tr = fs.as_struct(), ftr.as_struct()
            info = np.ascontiguousarray(self._fit.information, dtype=np.float64)
            mode = {"mean": 0, "marginal": 1, "joint": 2}[want]
            mean = np.empty(fs.n)
            second = None if mode == 0 else (np.empty(fs.n) if mode == 1 else np.empty((fs.n, fs.n), order="F"))
            ctx._check(ctx._lib.agp_solver_predict(ctx._h, ctx.kernel(cov), self._fit.train_covariance._solver(), C.byref(s_tr), _ptr(info),
                                                   C.byref(s_xs), _ptr(mean), None if second is None else _ptr(second), mode, capi.HOST),
                       "agp_solver_predict")
            mean = mean + m.mean_function_(fs.coords)  # mean_function_.add_to, gp.hpp:364
            if want == "mean":
                return mean
            return MarginalDistribution(mean, second) if want == "marginal" else JointDistribution(mean, second)
        # LinearCombination features on either side (callers.hpp:321-396): the same composition with the contracted covariance
        # matrices of agp_gram_combined, all of it in HBM (agp_solver_predict_combined)
        def side(f):
            if has_linear_combinations(f):
                ex, off, co = expand_with_offsets(f)
                return cov.features(ex), len(off) - 1, off, co
            fs_ = cov.features(f)
            return fs_, fs_.n, None, None
        ftr, ntr, troff, trco = side(self._fit.train_features)
        fxs, nxs, xoff, xco = side(features)
        s_tr, s_xs = ftr.as_struct(), fxs.as_struct()
        solver = self._fit.train_covariance._solver() if isinstance(self._fit, UpdatedGPFit) else self._fit._solver()
        info = np.ascontiguousarray(self._fit.information, dtype=np.float64)
        mode = {"mean": 0, "marginal": 1, "joint": 2}[want]
        mean = np.empty(nxs)
        second = None if mode == 0 else (np.empty(nxs) if mode == 1 else np.empty((nxs, nxs), order="F"))
        ctx._check(ctx._lib.agp_solver_predict_combined(
            ctx._h, ctx.kernel(cov), solver, C.byref(s_tr), ntr, None if troff is None else _ptr(troff), None if trco is None else _ptr(trco),
            _ptr(info), C.byref(s_xs), nxs, None if xoff is None else _ptr(xoff), None if xco is None else _ptr(xco), _ptr(mean),
            None if second is None else _ptr(second), mode, capi.HOST), "agp_solver_predict_combined")
        mean = mean + _mean_at(m.mean_function_, cov, features)  # mean_function_.add_to, gp.hpp:364
        if want == "mean":
            return mean
        return MarginalDistribution(mean, second) if want == "marginal" else JointDistribution(mean, second)

    def _xs(self, features):
        fs = self._model.covariance_function_.features(features)
        return fs, fs.as_struct()

    def _predict_mean(self, features):
        if isinstance(self._fit, UpdatedGPFit):
            return self._host_predict(features, "mean")
        m, ctx = self._model, self._model._ctx()
        fs, s = self._xs(features)
        mean = np.empty(fs.n)
        ctx._check(ctx._lib.agp_predict_mean(ctx._h, ctx.kernel(m.covariance_function_), self._fit._h, C.byref(s),
                                             _ptr(mean), capi.HOST), "agp_predict_mean")
        return mean + m.mean_function_(fs.coords)  # mean_function_.add_to, gp.hpp:364

    def _predict_marginal(self, features):
        if isinstance(self._fit, UpdatedGPFit):
            return self._host_predict(features, "marginal")
        m, ctx = self._model, self._model._ctx()
        fs, s = self._xs(features)
        mean, var = np.empty(fs.n), np.empty(fs.n)
        ctx._check(ctx._lib.agp_predict_marginal(ctx._h, ctx.kernel(m.covariance_function_), self._fit._h,
                                                 C.byref(s), _ptr(mean), _ptr(var), capi.HOST),
                   "agp_predict_marginal")
        return MarginalDistribution(mean + m.mean_function_(fs.coords), var)

    def _predict_joint(self, features):
        if isinstance(self._fit, UpdatedGPFit):
            return self._host_predict(features, "joint")
        m, ctx = self._model, self._model._ctx()
        fs, s = self._xs(features)
        mean, cov = np.empty(fs.n), np.empty((fs.n, fs.n), order="F")
        ctx._check(ctx._lib.agp_predict_joint(ctx._h, ctx.kernel(m.covariance_function_), self._fit._h, C.byref(s),
                                              _ptr(mean), _ptr(cov), capi.HOST), "agp_predict_joint")
        return JointDistribution(mean + m.mean_function_(fs.coords), cov)


    def _predict_joint_on_device(self, features):
        if isinstance(self._fit, UpdatedGPFit):
            raise NotImplementedError("joint(on_device=True) needs a fit that holds the plain LL^T factor")
        m, ctx = self._model, self._model._ctx()
        fs, s = self._xs(features)
        mean, cov = ctx.device_empty(fs.n), ctx.device_empty((fs.n, fs.n))
        ctx._check(ctx._lib.agp_predict_joint(ctx._h, ctx.kernel(m.covariance_function_), self._fit._h, C.byref(s),
                                              C.c_void_p(mean.ptr), C.c_void_p(cov.ptr), capi.DEVICE), "agp_predict_joint")
        # mean_function_.add_to (gp.hpp:364) on the m values of the mean; the m x m covariance is not moved
        return DeviceJointDistribution(ctx.to_device(mean.numpy() + m.mean_function_(fs.coords)), cov)


class GaussianProcessRegression:
    """GaussianProcessRegression<CovFunc, MeanFunc> (gp.hpp:487-505)."""

    def __init__(self, covariance_function, mean_function=None, model_name="gaussian_process_regression",
                 context=None):
        if not isinstance(covariance_function, CovarianceFunction):
            raise TypeError("covariance_function must be an albatross_amd CovarianceFunction")
        self.covariance_function_ = covariance_function
        self.mean_function_ = mean_function or ZeroMean()
        self.model_name_ = model_name
        self._context = context

    def _ctx(self):
        return self._context or default_context()

    def get_name(self):
        return self.model_name_

    def get_covariance(self):
        return self.covariance_function_

    def get_mean(self):
        return self.mean_function_

    # ParameterHandlingMixin subset (gp.hpp:255-268)
    def get_params(self):
        out = dict(self.covariance_function_.get_params())
        out.update(self.mean_function_.get_params())
        return out

    def set_param(self, name, value):
        if name in self.covariance_function_.get_params():
            self.covariance_function_.set_param(name, value)
        elif name in self.mean_function_.get_params():
            self.mean_function_.set_param(name, value)
        else:
            raise KeyError(name)

    def set_param_values(self, values):
        for k, v in values.items():
            self.set_param(k, v)

    set_params = set_param_values

    def _targets(self, fs, targets):
        y = np.ascontiguousarray(targets.mean - self.mean_function_(fs.coords), dtype=np.float64)  # remove_from
        yv = None
        if targets.covariance is not None:
            yv = np.ascontiguousarray(targets.covariance, dtype=np.float64)
            if yv.ndim != 1 or yv.shape[0] != y.shape[0]:
                raise ValueError("target covariance must be the diagonal (one variance per target)")
        if y.shape[0] != fs.n:
            raise ValueError("features and targets differ in size")
        return y, yv

    def fit(self, dataset, targets=None):
        """ModelBase::fit (core/model.hpp:137-152) -> _fit_impl (gp.hpp:281-294)."""
        if targets is not None:
            dataset = RegressionDataset(dataset, targets)
        ctx = self._ctx()
        if has_linear_combinations(dataset.features):
            return self._fit_dense(dataset)
        fs = self.covariance_function_.features(_values_of(dataset.features))
        y, yv = self._targets(fs, dataset.targets)
        s = fs.as_struct()
        h = C.c_void_p()
        if self.precision == "mixed":
            # agp_fit_create_mixed: fp32-product bulk updates + fp64 conjugate-gradient refinement of the
            # information vector (BASELINE configs[3]); `refinement_` keeps (iterations, relative residual)
            it, res = C.c_int(0), C.c_double(0.)
            st = ctx._lib.agp_fit_create_mixed(ctx._h, ctx.kernel(self.covariance_function_), C.byref(s), _ptr(y),
                                               _ptr(yv), int(self.max_refinements), float(self.refinement_tolerance),
                                               C.byref(h), None, None, C.byref(it), C.byref(res))
            self.refinement_ = (it.value, res.value)
        elif self.precision == "fp64":
            st = ctx._lib.agp_fit_create(ctx._h, ctx.kernel(self.covariance_function_), C.byref(s), _ptr(y), _ptr(yv),
                                         C.byref(h), None, None)
        else:
            raise ValueError(f"precision must be 'fp64' or 'mixed', not {self.precision!r}")
        if st != capi.AGP_OK:
            pivot = ctx._lib.agp_fit_failed_pivot(h) if h else -1
            if h:
                ctx._lib.agp_fit_destroy(h)
            if st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and self.pivoted_fallback:
                return self._fit_pivoted(dataset, fs, y, yv)
            ctx._check(st, f"agp_fit_create (pivot {pivot})")
        fit = GPFit(ctx, h, fs.n, dataset.features)
        fit.mixed_precision = self.precision == "mixed"
        return FitModel(self, fit)

    def fit_iterative(self, dataset, preconditioner_rank=256, preconditioner_tolerance=1e-12, tolerance=1e-10,
                      max_iterations=1000):
        """The exact fit that never forms the n x n covariance (albatross_amd/iterative.py: fit_iterative): an
        IterativeFitModel with .predict(features).mean() / .marginal()."""
        from .iterative import fit_iterative
        return fit_iterative(self, dataset, preconditioner_rank, preconditioner_tolerance, tolerance, max_iterations)

    pivoted_fallback = True
    # 'fp64' (the reference's arithmetic) or 'mixed' (fp32 MFMA products in the bulk updates of the factorisation,
    # information vector refined to fp64; see agp_fit_create_mixed in include/albatross_amd.h)
    precision = "fp64"
    max_refinements = 50
    refinement_tolerance = 1e-12
    refinement_ = None

    def _fit_pivoted(self, dataset, fs, y, yv):
        """The reference's own route for covariances that are only positive SEMI-definite ("unobservable" models,
        tests/test_gp.cc:20-33): Fit<GPFit<SerializableLDLT>> with the pivoted L D L^T (gp.hpp:61-69).  Gram and
        factor run on the device; predictions go through the generic CovarianceRepresentation form of
        _predict_impl.  Set `pivoted_fallback = False` to get NotPositiveDefiniteError instead."""
        ctx = self._ctx()
        feats = _values_of(dataset.features)
        K = ctx.gram(self.covariance_function_, Measurement(feats))  # as_measurements(features), gp.hpp:288-290
        if yv is not None:
            K[np.diag_indices_from(K)] += yv                          # gp.hpp:65
        if np.isnan(K).any():
            raise NanInputError(capi.AGP_ERR_NAN_INPUT, "covariance has NaN")  # gp.hpp:66
        ldlt = PivotedLDLT(K, ctx)                                    # gp.hpp:67
        return FitModel(self, UpdatedGPFit(feats, ldlt, ldlt.solve(y)))  # gp.hpp:68

    def _fit_dense(self, dataset):
        """Datasets with LinearCombination features: Fit<GPFit<SerializableLDLT>> (gp.hpp:61-69) from the contracted
        covariance matrix.  Gram of the expanded points, factorisation and solves run on the device; the
        contraction with the coefficients is host work."""
        ctx = self._ctx()
        feats = _values_of(dataset.features)
        y = np.ascontiguousarray(dataset.targets.mean - _mean_at(self.mean_function_, self.covariance_function_, feats))
        K = ctx.gram(self.covariance_function_, Measurement(feats))   # as_measurements(features), gp.hpp:288-290
        if dataset.targets.covariance is not None:
            K[np.diag_indices_from(K)] += np.asarray(dataset.targets.covariance, dtype=np.float64)  # gp.hpp:65
        if np.isnan(K).any():
            raise NanInputError(capi.AGP_ERR_NAN_INPUT, "covariance has NaN")                     # gp.hpp:66
        try:
            factor = DenseFactor(K, ctx)
        except NotPositiveDefiniteError:
            if not self.pivoted_fallback:
                raise
            factor = PivotedLDLT(K, ctx)
        return FitModel(self, UpdatedGPFit(feats, factor, factor.solve(y)))

    def ransac(self, strategy, *args, **kwargs):
        """ModelBase::ransac (ransac.hpp:507-524): model.ransac(strategy, inlier_threshold, random_sample_size,
        min_consensus_size, max_iterations[, max_failed_candidates]) or model.ransac(strategy, config) -> Ransac"""
        from .ransac import _model_ransac
        return _model_ransac(self, strategy, *args, **kwargs)

    def cross_validate(self):
        return CrossValidation(self)

    def fit_from_prediction(self, features, prediction):
        """fit_from_prediction (gp.hpp:236-245) -> gp_fit_from_prediction (gp.hpp:139-153): the model that
        reproduces a joint prediction at `features`: information = prior^-1 (mean - mean_function),
        train_covariance = ExplainedCovariance(prior_ldlt, prior - prediction.covariance)."""
        ctx = self._ctx()
        feats = _values_of(features)
        fs = self.covariance_function_.features(feats)
        mean = np.asarray(prediction.mean, dtype=np.float64) - self.mean_function_(fs.coords)  # remove_from, :240
        prior = ctx.gram(self.covariance_function_, feats)                                      # :243
        try:
            prior_ldlt = DenseFactor(prior, ctx)
        except NotPositiveDefiniteError:  # low-rank priors (tests/test_gp.cc:308-341): the pivoted factor
            prior_ldlt = PivotedLDLT(prior, ctx)
        cov = ExplainedCovariance(prior_ldlt, prior - np.asarray(prediction.covariance, dtype=np.float64))
        info = prior_ldlt.solve(mean)
        return FitModel(self, UpdatedGPFit(feats, cov, info))

    def log_likelihoods(self, dataset, parameter_sets):
        """log_likelihood(dataset) for several parameter vectors at once (agp_nll_batch): the evaluations
        compute_gradient (tune/finite_difference.hpp:20-94) and ModelTuner (tune/tune.hpp:151-161) make one
        after the other.  parameter_sets: iterable of {name: value} overrides of the current parameters.
        A parameter vector whose covariance is not positive definite gives NaN."""
        ctx = self._ctx()
        models = self._override_copies(parameter_sets)
        count = len(models)
        if count == 0:
            return np.zeros(0)
        feats = _values_of(dataset.features)
        fsets, structs, ys = [], [], []
        yv = None
        for m in models:
            fs = m.covariance_function_.features(feats)
            y, yv = m._targets(fs, dataset.targets)
            fsets.append(fs)
            structs.append(fs.as_struct())
            ys.append(y)
        n = fsets[0].n
        Y = np.asfortranarray(np.stack(ys, axis=1))
        # private handles for the duration of the call: the context's cache may evict while the batch is assembled
        handles = []
        try:
            for m in models:
                handles.append(ctx.private_kernel(m.covariance_function_))
            kernels = (C.c_void_p * count)(*handles)
            fptrs = (C.c_void_p * count)(*[C.addressof(st) for st in structs])
            out = np.empty(count)
            # log_likelihood ignores the target variance (gp.hpp:442-451): y_var = NULL
            ctx._check(ctx._lib.agp_nll_batch(ctx._h, count, kernels, fptrs, _ptr(Y), n, None, _ptr(out)),
                       "agp_nll_batch")
        finally:
            for kh in handles:
                ctx._lib.agp_kernel_destroy(kh)
        return -out

    def _override_copies(self, parameter_sets):
        """one copy of the model per {name: value} override dict, with its own covariance and mean functions"""
        import copy
        models = []
        for overrides in parameter_sets:
            m = copy.copy(self)
            m.covariance_function_ = copy.deepcopy(self.covariance_function_)
            m.mean_function_ = copy.deepcopy(self.mean_function_)
            m.set_param_values(overrides)
            models.append(m)
        return models

    def log_likelihood(self, dataset):
        """gp.hpp:442-451 (without priors: the parameter-prior subsystem is out of scope).  Like the reference, the
        covariance is covariance_function_(measurement_features) ALONE: dataset.targets.covariance is not added."""
        ctx = self._ctx()
        if has_linear_combinations(dataset.features):
            feats = _values_of(dataset.features)
            K = ctx.gram(self.covariance_function_, Measurement(feats))
            dev = dataset.targets.mean - _mean_at(self.mean_function_, self.covariance_function_, feats)
            return -negative_log_likelihood(dev, K, ctx)
        fs = self.covariance_function_.features(_values_of(dataset.features))
        y, _ = self._targets(fs, dataset.targets)
        s = fs.as_struct()
        out = C.c_double()
        ctx._check(ctx._lib.agp_nll(ctx._h, ctx.kernel(self.covariance_function_), C.byref(s), _ptr(y), None,
                                    C.byref(out)), "agp_nll")
        return -out.value


    def _slot_gradient(self, entry, dataset, with_variance):
        """One call of a gradient entry (agp_nll_gradient / agp_loo_nll_gradient) over the slot table of the covariance
        function: (value, slots, per-slot gradient, the n-vector the entry returns, the flattened features)"""
        p = _gradient_problem(self, dataset, entry)
        ctx = self._ctx()
        n = p.fs.n
        s = p.fs.as_struct()
        value = C.c_double()
        grad = np.zeros(len(p.slots))
        vec = np.empty(n)
        ctx._check(getattr(ctx._lib, entry)(ctx._h, ctx.kernel(self.covariance_function_), C.byref(s), _ptr(p.y),
                                            _ptr(p.yv) if with_variance else None, len(p.slots), p.table, _ptr(p.tangents), n,
                                            C.byref(value), _ptr(grad), _ptr(vec)),
                   entry)
        return value.value, p.slots, grad, vec, p.fs

    def _mean_tangent(self, fs, name):
        """d mu / d name at the features: a central difference of the mean function on the host"""
        import copy
        value = self.mean_function_.get_params()[name]
        h = 1e-6 * max(1.0, abs(value))
        up, down = copy.deepcopy(self.mean_function_), copy.deepcopy(self.mean_function_)
        up.set_param(name, value + h)
        down.set_param(name, value - h)
        return (np.asarray(up(fs.coords), dtype=np.float64) - np.asarray(down(fs.coords), dtype=np.float64)) / (2 * h)

    def log_likelihood_gradient(self, dataset):
        """(log_likelihood(dataset), {name: d log_likelihood / d name}) for every name of get_params(), exact to fp64
        rounding (agp_nll_gradient: one fit, K^-1 and a contraction against the derivative of the covariance program).
        The reference's tuner takes forward differences instead (compute_gradient, tune/finite_difference.hpp:37-90).
        As in log_likelihood, the target variance is not added and priors are not included.  ScalingTerm parameters
        go through the scaling function's d f / d name at the features (ScalingFunction.derivative), mean-function
        parameters through (d mu / d name)^T alpha with a central difference of the mean function on the host."""
        nll, slots, grad_nll, alpha, fs = self._slot_gradient("agp_nll_gradient", dataset, with_variance=False)
        return -nll, self._log_likelihood_gradient_dict(slots, grad_nll, alpha, fs)

    def _log_likelihood_gradient_dict(self, slots, grad_nll, alpha, fs):
        """{name: d log p / d name} from agp_nll_gradient's per-slot values and alpha (slots sharing a name summed)"""
        grad = {name: 0. for name in self.get_params()}
        for (_, _, name), g in zip(slots, grad_nll):
            grad[name] -= g
        # y = targets - mu: d log p / d theta = (d mu / d theta)^T alpha
        for name in self.mean_function_.get_params():
            grad[name] += float(self._mean_tangent(fs, name) @ alpha)
        return grad

    def log_likelihood_gradients(self, dataset, parameter_sets):
        """log_likelihood_gradient(dataset) for several parameter vectors at once (agp_nll_gradient_batch): the gradient
        counterpart of log_likelihoods, for the tuner's small problems where one exact gradient is a chain of small
        launches.  parameter_sets: iterable of {name: value} overrides of the current parameters (one model copy each,
        as log_likelihoods makes them).  Returns (log_likelihoods: array[count], gradients: [{name: value}] with every
        name of get_params()).  Sign, target variance and priors as in log_likelihood_gradient; ScalingTerm tangents
        are taken per copy, at its own parameters.  A parameter vector whose covariance is not positive definite (or
        has NaN) gives NaN throughout, not an exception.  fp64 models only."""
        if self.precision != "fp64":
            raise ValueError(f"log_likelihood_gradients: fp64 models only, not {self.precision!r}")
        models = self._override_copies(parameter_sets)
        if not models:
            return np.zeros(0), []
        lls, grads = _log_likelihood_gradients(self._ctx(), models, [dataset] * len(models))
        return np.asarray(lls), grads

    def leave_one_out_likelihood_gradient(self, dataset):
        """(LeaveOneOutLikelihood()(dataset, self), {name: d that / d name}) for every name of get_params(), exact to
        fp64 rounding (agp_loo_nll_gradient).  The value is the METRIC the tuner minimises, sum_i NLL_i of the
        leave-one-out predictions (evaluation/model_metrics.hpp:59-72), not a log-likelihood: log_likelihood_gradient
        returns +log p, this returns a sum of negative log-likelihoods.  Unlike log_likelihood, the target variance s is
        used, twice as the reference does: in the fit, and once more as the truth's variance of each score
        (v_i = 1 / (K^-1)_ii + s_i).  Priors are not included.  Parameters shared by several leaves are summed;
        ScalingTerm parameters go through ScalingFunction.derivative, mean-function parameters through -u^T d mu / d name
        (u = K^-1 a, the entry's mean weights) with a central difference of the mean function on the host.
        fp64 models only."""
        if self.precision != "fp64":
            raise ValueError(f"leave_one_out_likelihood_gradient: fp64 models only, not {self.precision!r}")
        loo, slots, grad_loo, u, fs = self._slot_gradient("agp_loo_nll_gradient", dataset, with_variance=True)
        return loo, self._leave_one_out_gradient_dict(slots, grad_loo, u, fs)

    def leave_one_out_likelihoods(self, dataset, parameter_sets):
        """LeaveOneOutLikelihood()(dataset, self) for several parameter vectors at once (agp_loo_nll_gradient_batch
        without slots: the value-only path, c_i from the column norms of R, no K^-1).  The counterpart of log_likelihoods
        for the metric: parameter_sets is an iterable of {name: value} overrides of the current parameters, the target
        variance is used as in leave_one_out_likelihood_gradient.  Returns an array of metric values; a parameter vector
        whose covariance is not positive definite (or has NaN) gives NaN.  fp64 models only."""
        if self.precision != "fp64":
            raise ValueError(f"leave_one_out_likelihoods: fp64 models only, not {self.precision!r}")
        models = self._override_copies(parameter_sets)
        if not models:
            return np.zeros(0)
        values, _ = _leave_one_out_likelihood_gradients(models, [dataset] * len(models), "leave_one_out_likelihoods", value_only=True)
        return np.asarray(values)

    def leave_one_out_likelihood_gradients(self, dataset, parameter_sets):
        """leave_one_out_likelihood_gradient(dataset) for several parameter vectors at once (agp_loo_nll_gradient_batch):
        the counterpart of log_likelihood_gradients for the metric the tuner minimises.  parameter_sets: iterable of
        {name: value} overrides of the current parameters (one model copy each).  Returns (values: array[count],
        gradients: [{name: value}] with every name of get_params()).  Signs, target variance and mean-function
        parameters as in leave_one_out_likelihood_gradient; ScalingTerm tangents are taken per copy, at its own
        parameters.  A parameter vector whose covariance is not positive definite (or has NaN) gives NaN throughout,
        not an exception.  fp64 models only."""
        if self.precision != "fp64":
            raise ValueError(f"leave_one_out_likelihood_gradients: fp64 models only, not {self.precision!r}")
        models = self._override_copies(parameter_sets)
        if not models:
            return np.zeros(0), []
        values, grads = _leave_one_out_likelihood_gradients(models, [dataset] * len(models), "leave_one_out_likelihood_gradients")
        return np.asarray(values), grads

    def leave_one_group_out_likelihood_gradient(self, dataset, grouper, predict_type="joint"):
        """(LeaveOneGroupOutLikelihood(grouper, predict_type)(dataset, self), {name: d that / d name}) for every name of
        get_params(), exact to fp64 rounding (agp_logo_nll_gradient_typed).  grouper: what CrossValidation.predict accepts -
        a callable on a feature, a LeaveOneOutGrouper or an indexer dict {key: [indices]}.  The value is the metric the
        tuner minimises, sum_g NLL_g of the held-out prediction of each group scored against the group's targets with their
        variances added (evaluation/model_metrics.hpp:74-93): predict_type "joint" scores against the group's full
        predictive covariance, "marginal" against its diagonal only (prediction_metrics.hpp:112-128).  The target variance
        is used twice, in the fit and in the score, as in leave_one_out_likelihood_gradient, and priors are not included.
        Parameters shared by several leaves are summed; ScalingTerm parameters go through ScalingFunction.derivative,
        mean-function parameters through -u^T d mu / d name (the entry's mean weights) with a central difference of the
        mean function on the host.  fp64 models only."""
        if self.precision != "fp64":
            raise ValueError(f"leave_one_group_out_likelihood_gradient: fp64 models only, not {self.precision!r}")
        ptype = _predict_type(predict_type)
        p = _gradient_problem(self, dataset, "agp_logo_nll_gradient")
        offsets, indices = _group_arrays(dataset, grouper, p.fs.n)
        ctx = self._ctx()
        n = p.fs.n
        s = p.fs.as_struct()
        value = C.c_double()
        grad = np.zeros(len(p.slots))
        u = np.empty(n)
        ctx._check(ctx._lib.agp_logo_nll_gradient_typed(ctx._h, ctx.kernel(self.covariance_function_), C.byref(s), _ptr(p.y), _ptr(p.yv),
                                                        len(offsets) - 1, _ptr(offsets), _ptr(indices), ptype, len(p.slots), p.table,
                                                        _ptr(p.tangents), n, C.byref(value), _ptr(grad), _ptr(u), None),
                   "agp_logo_nll_gradient_typed")
        return value.value, self._leave_one_out_gradient_dict(p.slots, grad, u, p.fs)

    def leave_one_group_out_likelihoods(self, dataset, grouper, parameter_sets, predict_type="joint"):
        """LeaveOneGroupOutLikelihood(grouper, predict_type)(dataset, self) for several parameter vectors at once
        (agp_logo_nll_gradient_batch without slots: the value alone, no H and no C B C).  parameter_sets: iterable of
        {name: value} overrides of the current parameters; grouper, predict_type and the target variance as in
        leave_one_group_out_likelihood_gradient.  Returns an array of metric values, NaN for a parameter vector whose
        covariance or one of whose group blocks is not positive definite (or has NaN).  fp64 models only."""
        models = self._override_copies(parameter_sets)
        if not models:
            return np.zeros(0)
        values, _, _ = _leave_one_group_out_likelihood_gradients(models, [dataset] * len(models), grouper, predict_type,
                                                                 "leave_one_group_out_likelihoods", value_only=True)
        return np.asarray(values)

    def leave_one_group_out_likelihood_gradients(self, dataset, grouper, parameter_sets, predict_type="joint"):
        """leave_one_group_out_likelihood_gradient(dataset, grouper, predict_type) for several parameter vectors at once
        (agp_logo_nll_gradient_batch): the counterpart of leave_one_out_likelihood_gradients for the grouped metric.
        Returns (values: array[count], gradients: [{name: value}] with every name of get_params()); NaN throughout for a
        parameter vector that fails.  fp64 models only."""
        models = self._override_copies(parameter_sets)
        if not models:
            return np.zeros(0), []
        values, grads, _ = _leave_one_group_out_likelihood_gradients(models, [dataset] * len(models), grouper, predict_type,
                                                                     "leave_one_group_out_likelihood_gradients")
        return np.asarray(values), grads

    def _leave_one_out_gradient_dict(self, slots, grad_loo, u, fs):
        """{name: d LOO / d name} from agp_loo_nll_gradient's per-slot values and mean weights u (slots sharing a name
        summed)"""
        grad = {name: 0. for name in self.get_params()}
        for (_, _, name), g in zip(slots, grad_loo):
            grad[name] += g
        # y = targets - mu: d LOO / d theta = -u^T (d mu / d theta)
        for name in self.mean_function_.get_params():
            grad[name] -= float(u @ self._mean_tangent(fs, name))
        return grad


class LeaveOneOutGrouper:
    """LeaveOneOutGrouper (indexing/group_by.hpp): every observation is its own group."""

    def __call__(self, feature, index=None):
        return index


def group_indexer(features, grouper):
    """dataset.group_by(grouper).indexers(): ordered {key: [indices]} (std::map order = sorted keys)."""
    feats = _values_of(features)
    groups = {}
    for i in range(len(feats)):
        key = i if isinstance(grouper, LeaveOneOutGrouper) else grouper(feats[i])
        groups.setdefault(key, []).append(i)
    return dict(sorted(groups.items(), key=lambda kv: kv[0]))


class CrossValidationPrediction:
    """Prediction<CrossValidation<Model>, Feature, GroupIndexer> (evaluation/cross_validation.hpp:28-260).

    means() / marginals() / joints() use the GP fast path (gp_cross_validated_predictions, gp.hpp:465-482:
    ONE fit, then held_out_predictions); predictions() is the generic refit-per-fold path."""

    def __init__(self, model, dataset, indexer):
        self.model_, self.dataset_, self.indexer_ = model, dataset, indexer
        self._fit_model = None

    def _fit(self):
        if self._fit_model is None:
            self._fit_model = self.model_.fit(self.dataset_)
        return self._fit_model.get_fit()

    def _held_out(self, joint):
        groups = list(self.indexer_.values())
        preds = self._fit().held_out_predictions(self.dataset_.targets.mean, groups, joint=joint)
        return dict(zip(self.indexer_.keys(), preds))

    def predictions(self):
        """predict_fold for every group: fit on the rest, predict the group (cross_validation.hpp:20-43)."""
        feats = _values_of(self.dataset_.features)
        y, yv = self.dataset_.targets.mean, self.dataset_.targets.covariance
        n = len(feats)
        out = {}
        for key, idx in self.indexer_.items():
            held = np.zeros(n, dtype=bool)
            held[np.asarray(idx)] = True
            train = np.nonzero(~held)[0]
            tr_feats = [feats[i] for i in train] if isinstance(feats, list) else feats[train]
            te_feats = [feats[i] for i in idx] if isinstance(feats, list) else feats[np.asarray(idx)]
            targets = MarginalDistribution(y[train], None if yv is None else yv[train])
            out[key] = self.model_.fit(RegressionDataset(tr_feats, targets)).predict(te_feats)
        return out

    def means(self):
        return {k: p.mean for k, p in self._held_out(False).items()}

    def marginals(self):
        return self._held_out(False)

    def joints(self):
        return self._held_out(True)

    def _concatenate(self, per_group):
        n = self.dataset_.size()
        out = np.empty(n)
        for key, idx in self.indexer_.items():
            out[np.asarray(idx)] = per_group[key]
        return out

    def mean(self):
        """concatenate_mean_predictions: group results scattered back to dataset order."""
        return self._concatenate(self.means())

    def marginal(self):
        m = self.marginals()
        return MarginalDistribution(self._concatenate({k: p.mean for k, p in m.items()}),
                                    self._concatenate({k: p.covariance for k, p in m.items()}))


class CrossValidation:
    """model.cross_validate() (core/model.hpp:154-156, evaluation/cross_validation.hpp:262-330)."""

    def __init__(self, model):
        self.model_ = model

    def predict(self, dataset, grouper):
        indexer = grouper if isinstance(grouper, dict) else group_indexer(dataset.features, grouper)
        return CrossValidationPrediction(self.model_, dataset, indexer)

    def predictions(self, dataset, grouper):
        return self.predict(dataset, grouper).predictions()

    def scores(self, metric, dataset, grouper):
        """cross_validated_scores: metric(prediction of the group, truth of the group) per group."""
        pred = self.predict(dataset, grouper)
        marg = pred.marginals()
        y = dataset.targets.mean
        return np.array([metric(marg[k], MarginalDistribution(y[np.asarray(idx)])) for k, idx in pred.indexer_.items()])


class LeaveOneOutLikelihood:
    """LeaveOneOutLikelihood<> (evaluation/model_metrics.hpp:59-72): metric(dataset, model) = sum over the points of the
    negative log-likelihood of each point's leave-one-out prediction, scored against the truth with its variance added
    (prediction_metrics.hpp:113-119).  No prior term.  One fit and R = L^-1 (agp_loo_nll_gradient, value only);
    model.leave_one_out_likelihood_gradient gives the gradient too."""

    def __call__(self, dataset, model):
        if model.precision != "fp64":
            raise ValueError(f"LeaveOneOutLikelihood: fp64 models only, not {model.precision!r}")
        if has_linear_combinations(dataset.features):
            raise NotImplementedError("LeaveOneOutLikelihood: LinearCombination features go through the dense path")
        ctx = model._ctx()
        cov = model.covariance_function_
        fs = cov.features(_values_of(dataset.features))
        y, yv = model._targets(fs, dataset.targets)
        s = fs.as_struct()
        out = C.c_double()
        ctx._check(ctx._lib.agp_loo_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(s), _ptr(y), _ptr(yv), 0, None, None, 0,
                                                 C.byref(out), None, None), "agp_loo_nll_gradient")
        return out.value


def _group_arrays(dataset, grouper, n):
    """(offsets, indices) int64 arrays of agp_logo_nll_gradient from what CrossValidation.predict accepts"""
    indexer = grouper if isinstance(grouper, dict) else group_indexer(dataset.features, grouper)
    groups = [np.asarray(idx, dtype=np.int64).reshape(-1) for idx in indexer.values()]
    offsets = np.zeros(len(groups) + 1, dtype=np.int64)
    if groups:
        offsets[1:] = np.cumsum([len(g) for g in groups])
    indices = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
    return offsets, np.ascontiguousarray(indices, dtype=np.int64)


_PREDICT_TYPES = {"joint": capi.PREDICT_JOINT, "marginal": capi.PREDICT_MARGINAL}


def _predict_type(predict_type):
    if predict_type not in _PREDICT_TYPES:
        raise ValueError(f"predict_type: 'joint' or 'marginal', not {predict_type!r}")
    return _PREDICT_TYPES[predict_type]


class LeaveOneGroupOutLikelihood:
    """LeaveOneGroupOutLikelihood<FeatureType, PredictType>(grouper) (evaluation/model_metrics.hpp:74-93):
    metric(dataset, model) = sum over the groups of the negative log-likelihood of the group's held-out prediction, scored
    against the group's targets with their variances added (prediction_metrics.hpp:112-128).  predict_type "joint" (the
    reference's default) scores against the full predictive covariance of the group, "marginal" against its diagonal only:
    the robust objective for large groups.  No prior term.  grouper: a callable on a feature, a LeaveOneOutGrouper or an
    indexer dict.  One fit, R = L^-1 and the group blocks from gathered columns of R (agp_logo_nll_gradient_typed, value
    only); group_scores gives the metric per group, model.leave_one_group_out_likelihood_gradient the gradient too."""

    def __init__(self, grouper, predict_type="joint"):
        self.grouper_ = grouper
        self.predict_type_ = predict_type
        _predict_type(predict_type)

    def _evaluate(self, dataset, model, per_group):
        if model.precision != "fp64":
            raise ValueError(f"LeaveOneGroupOutLikelihood: fp64 models only, not {model.precision!r}")
        if has_linear_combinations(dataset.features):
            raise NotImplementedError("LeaveOneGroupOutLikelihood: LinearCombination features go through the dense path")
        ctx = model._ctx()
        cov = model.covariance_function_
        fs = cov.features(_values_of(dataset.features))
        y, yv = model._targets(fs, dataset.targets)
        indexer = self.grouper_ if isinstance(self.grouper_, dict) else group_indexer(dataset.features, self.grouper_)
        offsets, indices = _group_arrays(dataset, indexer, fs.n)
        s = fs.as_struct()
        out = C.c_double()
        terms = np.zeros(len(indexer)) if per_group else None
        ctx._check(ctx._lib.agp_logo_nll_gradient_typed(ctx._h, ctx.kernel(cov), C.byref(s), _ptr(y), _ptr(yv), len(offsets) - 1,
                                                        _ptr(offsets), _ptr(indices), _predict_type(self.predict_type_), 0, None, None,
                                                        0, C.byref(out), None, None, _ptr(terms)),
                   "agp_logo_nll_gradient_typed")
        return out.value, indexer, terms

    def __call__(self, dataset, model):
        return self._evaluate(dataset, model, False)[0]

    def group_scores(self, dataset, model):
        """{group key: NLL_g} in indexer order (what cross_validated_scores returns for this metric, per group), from one
        value-only call: the per-group terms the device sums for __call__"""
        _, indexer, terms = self._evaluate(dataset, model, True)
        return {key: float(v) for key, v in zip(indexer.keys(), terms)}


def root_mean_square_error(prediction, truth):
    """RootMeanSquareError (evaluation/prediction_metrics.hpp)."""
    d = prediction.mean - truth.mean
    return float(np.sqrt(np.mean(d * d)))


RAGGED_CLASS_ROWS = 128  # the size classes of a ragged batch: ceil(n / 128), the row block of the factorisation


def _size_classes(sizes):
    """The problems of a ragged batch grouped by ceil(n_b / 128): a list of index lists, classes in ascending order, the
    indices of a class in the caller's order.  One lock-step call runs per class, padded to the class's largest size, so
    no problem is padded by 128 rows or more; equal sizes are one class without padding."""
    classes = {}
    for b, n in enumerate(sizes):
        classes.setdefault(-(-int(n) // RAGGED_CLASS_ROWS), []).append(b)
    return [classes[k] for k in sorted(classes)]


_BATCH_CALLS = itertools.count()  # serial numbers of the batched calls (GPFit._batch_origin)


def _padded_groups(ctx, fit_models):
    """The positions of fit_models grouped by the padded size of their fits (agp_fit_padded_size), groups in ascending
    order.  Inside a group the handles of one fit_batch / update_batch call come first, call by call in the order of
    their slots in the call's allocation (GPFit._batch_origin) - neighbours at one stride, which agp_predict_batch runs in
    lock step -, then the fits of calls of their own in the caller's order."""
    groups = {}
    for b, fm in enumerate(fit_models):
        groups.setdefault(int(ctx._lib.agp_fit_padded_size(fm._fit._h)), []).append(b)

    def origin(b):
        tag = getattr(fit_models[b]._fit, "_batch_origin", None)
        return (1, b, 0) if tag is None else (0,) + tag

    return [sorted(groups[k], key=origin) for k in sorted(groups)]


def fit_batch(models, datasets):
    """`models[b].fit(datasets[b])` for several problems in lock step (agp_fit_create_batch_ragged): the regime of the
    reference's own workloads (benchmarks/bench_predict.cc: N = 512; one fit per tuner step), where a single fit is bound by the
    latency of its serial pivots - a batch shares it.  models: GaussianProcessRegression objects on one context (one model
    may appear several times); datasets: as many RegressionDatasets.  Their sizes may differ: the problems are put into
    size classes (_size_classes) and one lock-step call runs per class, every problem padded with phantom rows to the
    largest size of its class; datasets of one size are one class without padding.  Returns the FitModels in the
    caller's order (rows() and information show the real rows); raises like `fit` for the first problem whose covariance
    has NaN or is not positive definite."""
    if len(models) != len(datasets) or not models:
        raise ValueError("fit_batch: as many datasets as models, at least one")
    ctx = models[0]._ctx()
    count = len(models)
    fsets, structs, ys, yvs = [], [], [], []
    for m, ds in zip(models, datasets):
        if m.precision != "fp64" or has_linear_combinations(ds.features) or m._ctx() is not ctx:
            raise ValueError("fit_batch: fp64 models on one context, plain features")
        fs = m.covariance_function_.features(_values_of(ds.features))
        y, yv = m._targets(fs, ds.targets)
        fsets.append(fs)
        structs.append(fs.as_struct())
        ys.append(y)
        yvs.append(yv)
    fits, statuses = [None] * count, [capi.AGP_OK] * count
    handles = []
    try:
        for m in models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(m.covariance_function_))
        for members in _size_classes([fs.n for fs in fsets]):
            k = len(members)
            n = max(fsets[b].n for b in members)  # the padded size of the class
            Y = np.zeros((n, k), order="F")
            have_var = any(yvs[b] is not None for b in members)
            V = np.zeros((n, k), order="F") if have_var else None
            for j, b in enumerate(members):
                Y[:fsets[b].n, j] = ys[b]
                if yvs[b] is not None:
                    V[:fsets[b].n, j] = yvs[b]
            out = (C.c_void_p * k)()
            status = (C.c_int * k)()
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            ctx._check(ctx._lib.agp_fit_create_batch_ragged(ctx._h, k, kernels, fptrs, _ptr(Y), n, _ptr(V) if have_var else None, n,
                                                            out, None, 0, None, status), "agp_fit_create_batch_ragged")
            call = next(_BATCH_CALLS)
            for j, b in enumerate(members):
                fits[b] = GPFit(ctx, C.c_void_p(out[j]), fsets[b].n, datasets[b].features)
                fits[b]._batch_origin = (call, j)
                statuses[b] = status[j]
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    for b in range(count):  # the caller's index, whatever class the problem ran in
        if statuses[b] != capi.AGP_OK:
            pivot = ctx._lib.agp_fit_failed_pivot(fits[b]._h)
            ctx._check(statuses[b], f"agp_fit_create_batch: problem {b} (pivot {pivot})")
    return [FitModel(m, f) for m, f in zip(models, fits)]


def predict_batch(fit_models, features, what="marginal"):
    """`fit_models[b].predict(features[b])` for several fits in lock step (agp_predict_batch): what follows
    fit_batch - at a few hundred points one prediction is a handful of latency-bound launches, a batch runs each once.
    fit_models: FitModels holding plain GPFits on one context (the handles of fit_batch or update_batch, or any mix of
    fits: they are grouped by padded size, one call runs per group, and inside it neighbours whose factors lie at one
    stride are predicted together, the others one by one).  features: ONE array
    shared by all problems, or a list with one entry per model, every entry with the same number of points;
    Measurement-wrapped features behave as in predict_with_measurement_noise.  what: "mean" | "marginal" | "joint".
    Returns a list of mean arrays, MarginalDistributions or JointDistributions, each with its model's mean function
    added back (gp.hpp:346,364)."""
    modes = {"mean": 0, "marginal": 1, "joint": 2}
    if what not in modes:
        raise ValueError(f"predict_batch: what must be one of {sorted(modes)}, not {what!r}")
    fit_models = list(fit_models)
    count = len(fit_models)
    if count == 0:
        raise ValueError("predict_batch: at least one fit model")
    if has_linear_combinations(features):
        raise ValueError("predict_batch: LinearCombination features are not supported (predict one model at a time)")
    shared = not isinstance(features, (list, tuple))  # an array, a Measurement or a FeatureSet: one vector for all problems
    per_model = [features] * count if shared else list(features)
    if len(per_model) != count:
        raise ValueError("predict_batch: one feature vector per fit model (or one shared by all)")
    for fm in fit_models:
        if not isinstance(fm, FitModel) or type(fm._fit) is not GPFit or fm._fit.mixed_precision:
            raise ValueError("predict_batch: every fit must be a plain fp64 GPFit (fit / fit_batch)")
    ctx = fit_models[0]._model._ctx()
    fsets = []
    for fm, f in zip(fit_models, per_model):
        if fm._model._ctx() is not ctx:
            raise ValueError("predict_batch: every fit model must live on one context")
        if has_linear_combinations(f):
            raise ValueError("predict_batch: LinearCombination features are not supported (predict one model at a time)")
        fsets.append(fm._model.covariance_function_.features(f))
    m = fsets[0].n
    if any(fs.n != m for fs in fsets):
        raise ValueError("predict_batch: every feature vector must have the same number of points")
    mode = modes[what]
    structs = [fs.as_struct() for fs in fsets]
    mean = np.empty((m, count), order="F")
    second = None if mode == 0 else np.empty((m if mode == 1 else m * m, count), order="F")
    statuses = [capi.AGP_OK] * count
    handles = []
    try:
        for fm in fit_models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(fm._model.covariance_function_))
        groups = _padded_groups(ctx, fit_models)
        for members in groups:
            k = len(members)
            whole = k == count and members == list(range(count))  # one group in the caller's order: results land in place
            g_mean = mean if whole else np.empty((m, k), order="F")
            g_second = second if whole or second is None else np.empty((second.shape[0], k), order="F")
            status = (C.c_int * k)()
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            fits = (C.c_void_p * k)(*[fit_models[b]._fit._h.value for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            ctx._check(ctx._lib.agp_predict_batch(ctx._h, k, kernels, fits, fptrs, mode, _ptr(g_mean), max(m, 1),
                                                  None if g_second is None else _ptr(g_second),
                                                  max(g_second.shape[0], 1) if g_second is not None else 0, capi.HOST, status),
                       "agp_predict_batch")
            for j, b in enumerate(members):
                statuses[b] = status[j]
                if not whole:
                    mean[:, b] = g_mean[:, j]
                    if second is not None:
                        second[:, b] = g_second[:, j]
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    for b in range(count):
        ctx._check(statuses[b], f"agp_predict_batch: problem {b}")
    out = []
    for b, (fm, fs) in enumerate(zip(fit_models, fsets)):
        mu = mean[:, b] + fm._model.mean_function_(fs.coords)  # mean_function_.add_to
        if mode == 0:
            out.append(mu)
        elif mode == 1:
            out.append(MarginalDistribution(mu, second[:, b].copy()))
        else:
            out.append(JointDistribution(mu, second[:, b].reshape((m, m), order="F").copy(order="F")))
    return out


def update_batch(fit_models, datasets):
    """`fit_models[b].update(datasets[b])` for several fits in lock step (agp_fit_update_batch): the third verb
    after fit_batch and predict_batch - a caller who keeps many small models and conditions each on every new epoch of
    observations pays the launch chain of an update once per batch, not once per model.  fit_models: FitModels holding
    plain fp64 GPFits on one context (of fit, fit_batch, update or update_batch, in any mix and of any sizes: they are
    grouped by padded size and one call runs per group); datasets: as
    many RegressionDatasets, each with the same number of points.  Each model's mean function is removed from its
    targets.  Returns the FitModels of the grown fits (rows() == old + m, training features concatenated); raises like
    `update` for the first problem whose covariance has NaN or is not positive definite, after destroying every handle."""
    fit_models, datasets = list(fit_models), list(datasets)
    count = len(fit_models)
    if count == 0:
        raise ValueError("update_batch: at least one fit model")
    if len(datasets) != count:
        raise ValueError("update_batch: as many datasets as fit models")
    for fm in fit_models:
        if not isinstance(fm, FitModel) or type(fm._fit) is not GPFit or fm._fit.mixed_precision:
            raise ValueError("update_batch: every fit must be a plain fp64 GPFit (fit / fit_batch / update)")
    ctx = fit_models[0]._model._ctx()
    feats, fsets = [], []
    for fm, ds in zip(fit_models, datasets):
        if fm._model._ctx() is not ctx:
            raise ValueError("update_batch: every fit model must live on one context")
        f = _values_of(ds.features)
        if has_linear_combinations(f) or has_linear_combinations(fm._fit.train_features):
            raise ValueError("update_batch: LinearCombination features are not supported (update one model at a time)")
        feats.append(f)
        fsets.append(fm._model.covariance_function_.features(f))
    m = fsets[0].n
    if any(fs.n != m for fs in fsets):
        raise ValueError("update_batch: every dataset must have the same number of points")
    ys, yvs = [], []
    for fm, fs, ds in zip(fit_models, fsets, datasets):
        y, yv = fm._model._targets(fs, ds.targets)  # mean function removed (ModelBase::update -> remove_from)
        ys.append(y)
        yvs.append(yv)
    structs = [fs.as_struct() for fs in fsets]
    handles = []
    out = [None] * count
    statuses = [capi.AGP_OK] * count
    origins = [None] * count

    def destroy_all():
        for h in out:
            if h:
                ctx._lib.agp_fit_destroy(C.c_void_p(h))

    try:
        for fm in fit_models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(fm._model.covariance_function_))
        for members in _padded_groups(ctx, fit_models):
            k = len(members)
            Y = np.asfortranarray(np.stack([ys[b] for b in members], axis=1))
            have_var = any(yvs[b] is not None for b in members)
            V = np.asfortranarray(np.stack([np.zeros(m) if yvs[b] is None else yvs[b] for b in members], axis=1)) if have_var else None
            g_out = (C.c_void_p * k)()
            status = (C.c_int * k)()
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            olds = (C.c_void_p * k)(*[fit_models[b]._fit._h.value for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            try:
                ctx._check(ctx._lib.agp_fit_update_batch(ctx._h, k, kernels, olds, fptrs, _ptr(Y), m, _ptr(V) if have_var else None, m,
                                                         g_out, None, 0, None, status), "agp_fit_update_batch")
            except Exception:
                destroy_all()  # (the grown fits of the groups before this one)
                raise
            call = next(_BATCH_CALLS)
            for j, b in enumerate(members):
                out[b] = g_out[j]
                statuses[b] = status[j]
                origins[b] = (call, j)
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    for b in range(count):
        if statuses[b] != capi.AGP_OK:
            pivot = ctx._lib.agp_fit_failed_pivot(C.c_void_p(out[b]))
            destroy_all()
            ctx._check(statuses[b], f"agp_fit_update_batch: problem {b} (pivot {pivot})")
    grown = []
    for b, (fm, fs) in enumerate(zip(fit_models, fsets)):
        old_feats = _values_of(fm._fit.train_features)
        try:
            new_feats = np.concatenate([np.asarray(old_feats, dtype=np.float64).reshape(fm._fit.rows(), -1),
                                        np.asarray(feats[b], dtype=np.float64).reshape(fs.n, -1)])
        except (TypeError, ValueError):  # feature containers numpy cannot stack: keep them side by side
            new_feats = (old_feats, feats[b])
        grown.append(FitModel(fm._model, GPFit(ctx, C.c_void_p(out[b]), fm._fit.rows() + fs.n, new_feats)))
        grown[-1]._fit._batch_origin = origins[b]
    return grown


class _GradientProblem:
    """the host side of one gradient problem: flattened features, targets (mean removed) and variances, the slot table
    of the covariance function (param_slots), its ctypes form and the tangent columns (n x columns, column-major) of
    its ScalingTerm slots at the function's current parameters (None without such slots)"""

    def __init__(self, fs, y, yv, slots, table, tangents):
        self.fs, self.y, self.yv, self.slots, self.table, self.tangents = fs, y, yv, slots, table, tangents


def _gradient_problem(model, dataset, entry="agp_nll_gradient"):
    """_GradientProblem of `model` on `dataset`: what agp_nll_gradient, agp_loo_nll_gradient and agp_nll_gradient_batch
    are given for it"""
    if has_linear_combinations(dataset.features):
        raise NotImplementedError(f"{entry}: LinearCombination features go through the dense path")
    cov = model.covariance_function_
    fs = cov.features(_values_of(dataset.features))
    y, yv = model._targets(fs, dataset.targets)
    slots, columns = cov.param_slots()
    if len(slots) > capi.MAX_GRADIENT_SLOTS:
        raise ValueError(f"more than {capi.MAX_GRADIENT_SLOTS} covariance parameter slots")
    tangents = None
    if columns:
        tangents = np.empty((fs.n, len(columns)), order="F")
        for c, (fn, name) in enumerate(columns):
            tangents[:, c] = fn.derivative(fs.coords, name)
    table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(node, p) for node, p, _ in slots])
    return _GradientProblem(fs, y, yv, slots, table, tangents)


def _ragged_columns(problems, members, n, column):
    """the n x len(members) column-major array whose column j holds column(problems[members[j]]) - n_b values, zeros
    behind them - or None when no member has that vector (a member without one keeps its zeros)"""
    vectors = [column(problems[b]) for b in members]
    if all(v is None for v in vectors):
        return None
    out = np.zeros((n, len(members)), order="F")
    for j, v in enumerate(vectors):
        if v is not None:
            out[:len(v), j] = v
    return out


def _ragged_tangents(problems, members, n):
    """the tangent columns of the members at the leading dimension n of their call (the padded size): the problem's own
    array where it has n rows already, else a copy with zeros behind the n_b values.  Returns (pointer array, the arrays
    to keep alive)."""
    keep = []
    for b in members:
        t = problems[b].tangents
        if t is not None and t.shape[0] != n:
            wide = np.zeros((n, t.shape[1]), order="F")
            wide[:t.shape[0]] = t
            t = wide
        keep.append(t)
    return (C.c_void_p * len(members))(*[None if t is None else t.ctypes.data for t in keep]), keep


def _log_likelihood_gradients(ctx, models, datasets):
    """models[b] on datasets[b], of any mix of sizes: one agp_nll_gradient_batch_ragged call per size class
    (_size_classes; datasets of one size are one class and run the launches of agp_nll_gradient_batch).  Returns
    ([log p_b], [{name: d log p_b / d name}]) in the caller's order, NaN throughout for a problem whose covariance has NaN
    or is not positive definite"""
    count = len(models)
    for m, ds in zip(models, datasets):
        if m.precision != "fp64" or m._ctx() is not ctx:
            raise ValueError("log_likelihood_gradient_batch: fp64 models on one context")
    problems = [_gradient_problem(m, ds, "agp_nll_gradient_batch") for m, ds in zip(models, datasets)]
    structs = [p.fs.as_struct() for p in problems]
    lls, grads = [None] * count, [None] * count
    handles = []
    try:
        for m in models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(m.covariance_function_))
        for members in _size_classes([p.fs.n for p in problems]):
            k = len(members)
            n = max(problems[b].fs.n for b in members)  # the padded size of the class
            Y = _ragged_columns(problems, members, n, lambda p: p.y)
            ldg = max(1, max(len(problems[b].slots) for b in members))
            nll = np.empty(k)
            grad = np.zeros((k, ldg))   # column j of the ldg x k array: row j here
            alpha = np.zeros((k, n))    # likewise, ldi = n; problem b's n_b values lead its row
            status = (C.c_int * k)()
            n_slots = (C.c_int * k)(*[len(problems[b].slots) for b in members])
            tables = (C.c_void_p * k)(*[C.addressof(problems[b].table) for b in members])
            tangents, _keep = _ragged_tangents(problems, members, n)
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            # log_likelihood ignores the target variance (gp.hpp:442-451): y_var = NULL
            ctx._check(ctx._lib.agp_nll_gradient_batch_ragged(ctx._h, k, kernels, fptrs, _ptr(Y), n, None, 0, n_slots, tables,
                                                              tangents, n, _ptr(nll), _ptr(grad), ldg, _ptr(alpha), n, status),
                       f"agp_nll_gradient_batch_ragged: problems {members}")
            for j, b in enumerate(members):
                m, p = models[b], problems[b]
                if status[j] != capi.AGP_OK:
                    lls[b] = float("nan")
                    grads[b] = {name: float("nan") for name in m.get_params()}
                    continue
                lls[b] = -nll[j]
                grads[b] = m._log_likelihood_gradient_dict(p.slots, grad[j, :len(p.slots)], alpha[j, :p.fs.n], p.fs)
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    return lls, grads


def log_likelihood_gradient_batch(models, datasets):
    """`models[b].log_likelihood_gradient(datasets[b])` for several INDEPENDENT problems in lock step
    (agp_nll_gradient_batch_ragged): the gradient counterpart of fit_batch, for multi-start tuning and one model per
    station / group.  models: fp64 GaussianProcessRegression objects on one context (their covariance trees and feature
    dimensions may differ; one model may appear several times); datasets: as many RegressionDatasets.  Their sizes may
    differ: the problems are put into size classes (_size_classes) and one lock-step call runs per class, every problem
    padded with phantom rows to the largest size of its class; equal sizes are one class without padding.
    Returns a list of (log_likelihood, {name: gradient}) in the caller's order; a problem whose covariance has NaN or is
    not positive definite gives NaN throughout instead of raising."""
    if len(models) != len(datasets) or not models:
        raise ValueError("log_likelihood_gradient_batch: as many datasets as models, at least one")
    lls, grads = _log_likelihood_gradients(models[0]._ctx(), list(models), list(datasets))
    return list(zip(lls, grads))


def _leave_one_out_likelihood_gradients(models, datasets, caller, value_only=False):
    """models[b] on datasets[b], of any mix of sizes: one agp_loo_nll_gradient_batch_ragged call per size class.  Returns
    ([LOO_b], [{name: d LOO_b / d name}]) in the caller's order, NaN throughout for a problem whose covariance has NaN or
    is not positive definite.  caller: the public name, for the error texts.  value_only: no slots and no mean weights
    (the entry's value-only path); the gradients are None."""
    count = len(models)
    # plain checks first, none of which needs a device: LinearCombination features, precision, then one context
    for ds in datasets:
        if has_linear_combinations(ds.features):
            raise NotImplementedError(f"{caller} (agp_loo_nll_gradient_batch): LinearCombination features go through the dense path")
    if any(m.precision != "fp64" for m in models):
        raise ValueError(f"{caller}: fp64 models only")
    ctx = models[0]._ctx()
    if any(m._ctx() is not ctx for m in models):
        raise ValueError(f"{caller}: every model must live on one context")
    problems = [_gradient_problem(m, ds, "agp_loo_nll_gradient_batch") for m, ds in zip(models, datasets)]
    structs = [p.fs.as_struct() for p in problems]
    values, grads = [None] * count, [None] * count
    handles = []
    try:
        for m in models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(m.covariance_function_))
        for members in _size_classes([p.fs.n for p in problems]):
            k = len(members)
            n = max(problems[b].fs.n for b in members)  # the padded size of the class
            Y = _ragged_columns(problems, members, n, lambda p: p.y)
            # the target variance, in the fit and as the truth's variance; problems without one get zeros beside those with one
            V = _ragged_columns(problems, members, n, lambda p: p.yv)
            n_used = [0 if value_only else len(problems[b].slots) for b in members]
            ldg = max(1, max(n_used))
            loo = np.empty(k)
            grad = np.zeros((k, ldg))                      # column j of the ldg x k array: row j here
            u = None if value_only else np.zeros((k, n))  # likewise, ldw = n
            status = (C.c_int * k)()
            n_slots = (C.c_int * k)(*n_used)
            tables = (C.c_void_p * k)(*[C.addressof(problems[b].table) for b in members])
            tangents, _keep = _ragged_tangents(problems, members, n)
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            ctx._check(ctx._lib.agp_loo_nll_gradient_batch_ragged(ctx._h, k, kernels, fptrs, _ptr(Y), n,
                                                                  None if V is None else _ptr(V), n, n_slots, tables, tangents, n,
                                                                  _ptr(loo), _ptr(grad), ldg, None if value_only else _ptr(u), n,
                                                                  status),
                       f"agp_loo_nll_gradient_batch_ragged: problems {members}")
            for j, b in enumerate(members):
                m, p = models[b], problems[b]
                ok = status[j] == capi.AGP_OK
                values[b] = float(loo[j]) if ok else float("nan")
                if value_only:
                    grads[b] = None
                elif ok:
                    grads[b] = m._leave_one_out_gradient_dict(p.slots, grad[j, :len(p.slots)], u[j, :p.fs.n], p.fs)
                else:
                    grads[b] = {name: float("nan") for name in m.get_params()}
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    return values, grads


def leave_one_out_likelihood_gradient_batch(models, datasets):
    """`models[b].leave_one_out_likelihood_gradient(datasets[b])` for several INDEPENDENT problems in lock step
    (agp_loo_nll_gradient_batch_ragged): the counterpart of log_likelihood_gradient_batch for the leave-one-out metric.
    models: fp64 GaussianProcessRegression objects on one context (their covariance trees and feature dimensions may
    differ); datasets: as many RegressionDatasets of any mix of sizes (one call per size class, as
    log_likelihood_gradient_batch), each with or without a target variance.  Returns a list of (value, {name: gradient})
    in the caller's order; a problem whose covariance has NaN or is not positive definite gives NaN throughout instead of
    raising."""
    if len(models) != len(datasets) or not models:
        raise ValueError("leave_one_out_likelihood_gradient_batch: as many datasets as models, at least one")
    values, grads = _leave_one_out_likelihood_gradients(list(models), list(datasets), "leave_one_out_likelihood_gradient_batch")
    return list(zip(values, grads))


def _leave_one_group_out_likelihood_gradients(models, datasets, grouper, predict_type, caller, value_only=False):
    """models[b] on datasets[b], of any mix of sizes, each with its own groups: one agp_logo_nll_gradient_batch call per
    size class.  grouper: one for every dataset, or a list / tuple with one per dataset.  Returns ([LOGO_b],
    [{name: d LOGO_b / d name}], [status_b]) in the caller's order, NaN throughout for a problem that failed (its covariance
    or a group block not positive definite, NaN input).  value_only: no slots and no mean weights; the gradients are None."""
    count = len(models)
    ptype = _predict_type(predict_type)
    for ds in datasets:
        if has_linear_combinations(ds.features):
            raise NotImplementedError(f"{caller} (agp_logo_nll_gradient_batch): LinearCombination features go through the dense path")
    if any(m.precision != "fp64" for m in models):
        raise ValueError(f"{caller}: fp64 models only")
    ctx = models[0]._ctx()
    if any(m._ctx() is not ctx for m in models):
        raise ValueError(f"{caller}: every model must live on one context")
    groupers = list(grouper) if isinstance(grouper, (list, tuple)) else [grouper] * count
    if len(groupers) != count:
        raise ValueError(f"{caller}: one grouper, or one per dataset")
    problems = [_gradient_problem(m, ds, "agp_logo_nll_gradient_batch") for m, ds in zip(models, datasets)]
    groups = [_group_arrays(ds, gr, p.fs.n) for ds, gr, p in zip(datasets, groupers, problems)]  # (offsets, indices)
    structs = [p.fs.as_struct() for p in problems]
    values, grads, statuses = [None] * count, [None] * count, [None] * count
    handles = []
    try:
        for m in models:  # private handles: the context's small kernel cache may evict while the batch is assembled
            handles.append(ctx.private_kernel(m.covariance_function_))
        for members in _size_classes([p.fs.n for p in problems]):
            k = len(members)
            n = max(problems[b].fs.n for b in members)  # the padded size of the class
            Y = _ragged_columns(problems, members, n, lambda p: p.y)
            V = _ragged_columns(problems, members, n, lambda p: p.yv)
            n_used = [0 if value_only else len(problems[b].slots) for b in members]
            ldg = max(1, max(n_used))
            logo = np.empty(k)
            grad = np.zeros((k, ldg))                      # column j of the ldg x k array: row j here
            u = None if value_only else np.zeros((k, n))  # likewise, ldw = n
            status = (C.c_int * k)()
            n_slots = (C.c_int * k)(*n_used)
            n_groups = (C.c_int64 * k)(*[len(groups[b][0]) - 1 for b in members])
            offsets = (C.c_void_p * k)(*[groups[b][0].ctypes.data for b in members])
            indices = (C.c_void_p * k)(*[groups[b][1].ctypes.data for b in members])
            tables = (C.c_void_p * k)(*[C.addressof(problems[b].table) for b in members])
            tangents, _keep = _ragged_tangents(problems, members, n)
            kernels = (C.c_void_p * k)(*[handles[b] for b in members])
            fptrs = (C.c_void_p * k)(*[C.addressof(structs[b]) for b in members])
            ctx._check(ctx._lib.agp_logo_nll_gradient_batch(ctx._h, k, kernels, fptrs, _ptr(Y), n, None if V is None else _ptr(V), n,
                                                            n_groups, offsets, indices, ptype, n_slots, tables, tangents, n,
                                                            _ptr(logo), _ptr(grad), ldg, None if value_only else _ptr(u), n, None,
                                                            status),
                       f"agp_logo_nll_gradient_batch: problems {members}")
            for j, b in enumerate(members):
                m, p = models[b], problems[b]
                statuses[b] = int(status[j])
                ok = status[j] == capi.AGP_OK
                values[b] = float(logo[j]) if ok else float("nan")
                if value_only:
                    grads[b] = None
                elif ok:
                    grads[b] = m._leave_one_out_gradient_dict(p.slots, grad[j, :len(p.slots)], u[j, :p.fs.n], p.fs)
                else:
                    grads[b] = {name: float("nan") for name in m.get_params()}
    finally:
        for kh in handles:
            ctx._lib.agp_kernel_destroy(kh)
    return values, grads, statuses


def leave_one_group_out_likelihood_gradient_batch(models, datasets, grouper, predict_type="joint"):
    """`models[b].leave_one_group_out_likelihood_gradient(datasets[b], grouper_b, predict_type)` for several INDEPENDENT
    problems in lock step (agp_logo_nll_gradient_batch): the counterpart of leave_one_out_likelihood_gradient_batch for the
    metric to tune with when observations come in correlated bunches.  models: fp64 GaussianProcessRegression objects on one
    context; datasets: as many RegressionDatasets of any mix of sizes (one call per size class); grouper: one for all, or a
    list / tuple with one per dataset (what leave_one_group_out_likelihood_gradient accepts).  The group blocks of all
    problems of a call run as one chain per size class of groups.  Returns a list of (value, {name: gradient}, status) in
    the caller's order; a problem that fails (status != 0: its covariance or one of its group blocks is not positive
    definite, or its input has NaN) gives NaN throughout instead of raising."""
    if len(models) != len(datasets) or not models:
        raise ValueError("leave_one_group_out_likelihood_gradient_batch: as many datasets as models, at least one")
    values, grads, statuses = _leave_one_group_out_likelihood_gradients(list(models), list(datasets), grouper, predict_type,
                                                                        "leave_one_group_out_likelihood_gradient_batch")
    return list(zip(values, grads, statuses))


def _pooled(model, results):
    """(sum of the values, {name: sum of the gradients}) of the per-dataset results of one model, summed in the caller's
    order; NaN throughout if any problem failed"""
    names = list(model.get_params())
    results = [r[:2] for r in results]
    if any(np.isnan(v) for v, _ in results):
        return float("nan"), {name: float("nan") for name in names}
    total = 0.
    grad = {name: 0. for name in names}
    for v, g in results:
        total += v
        for name in names:
            grad[name] += g[name]
    return total, grad


def pooled_log_likelihood_gradient(model, datasets):
    """One model shared by many datasets of any sizes (one parameter vector tuned on every station's data):
    (sum_b log p_b, {name: sum_b d log p_b / d name}) over log_likelihood_gradient_batch([model] * B, datasets).  NaN
    throughout if any problem fails."""
    datasets = list(datasets)
    return _pooled(model, log_likelihood_gradient_batch([model] * len(datasets), datasets))


def pooled_leave_one_out_likelihood_gradient(model, datasets):
    """pooled_log_likelihood_gradient for the leave-one-out metric: (sum_b LOO_b, {name: sum_b d LOO_b / d name}) over
    leave_one_out_likelihood_gradient_batch([model] * B, datasets).  NaN throughout if any problem fails."""
    datasets = list(datasets)
    return _pooled(model, leave_one_out_likelihood_gradient_batch([model] * len(datasets), datasets))


def pooled_leave_one_group_out_likelihood_gradient(model, datasets, grouper, predict_type="joint"):
    """pooled_log_likelihood_gradient for the leave-one-group-out metric: (sum_b LOGO_b, {name: sum_b d LOGO_b / d name})
    over leave_one_group_out_likelihood_gradient_batch([model] * B, datasets, grouper, predict_type).  NaN throughout if
    any problem fails."""
    datasets = list(datasets)
    return _pooled(model, leave_one_group_out_likelihood_gradient_batch([model] * len(datasets), datasets, grouper, predict_type))


def gp_from_covariance(covariance_function, model_name="gaussian_process_regression", context=None):
    """gp.hpp:507-521"""
    return GaussianProcessRegression(covariance_function, None, model_name, context)


def gp_from_covariance_and_mean(covariance_function, mean_function, model_name="gaussian_process_regression",
                                context=None):
    """gp.hpp:523-537"""
    return GaussianProcessRegression(covariance_function, mean_function, model_name, context)
